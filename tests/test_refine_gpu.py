"""GPU tests of the depth refinement entry point (p2p_refine_depth_batch, csrc/icp.hip) at 640 x 480 with L-mesh frames: against the
host chain icp_inputs_batch -> tests/icp_ref.py -> composition (icp_refinement :91-93) -> the depth score; its score and inlier mask
against depth_score_batch at the pose it returned (bit for bit); the gated statuses; a known-pose recovery; 256 jobs over 4 frames and
alone against in a batch.

Bars: status, iterations and pairs exact; R entries within 1e-9 and t within 1e-6 mm of the host chain (the ICP pose bar of
tests/test_icp_gpu.py carried through the composition).  Known-pose recovery: with the union mask equal to the object's silhouette,
the refined pose is closer to the true one than the pose the ICP starts from (job.R and t_adjusted), in rotation and in translation,
and within the restatement's own error + 0.01 deg / 0.05 mm.  (A union mask grown into the background pulls the centroid shift, and so
the ICP's start, about 40 mm off the object; the restatement measured on the host: 3.0-5.7 mm at t_adjusted -> 0.2-3.4 mm, and
0.45-4.0 deg -> 0.04-0.78 deg.)"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_ref as D  # noqa: E402
import icp_ref as I  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 480, 640
K = D.K_640


@pytest.fixture(scope="module")
def ctx():
    from pix2pose_amd.runtime import Context
    c = Context(0, max_batch=8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def mesh(ctx):
    from pix2pose_amd.runtime import Mesh
    v, t = D.l_mesh(8)
    return Mesh(ctx, v, t)


def true_pose(k):
    R = D.rot(0, 20 + 7 * k) @ D.rot(1, -25 + 11 * k) @ D.rot(2, 5 * k)
    t = np.array([-40.0 + 25 * k, 20.0 - 10 * k, 650.0 + 30 * k])
    return R, t


def frame(ctx, mesh, k, seed):
    """A sensor frame: a wavy wall with the L mesh at true_pose(k) in front of it, sensor noise and dropout."""
    from pix2pose_amd import runtime
    R, t = true_pose(k)
    obj = runtime.render_depth_batch(ctx, [mesh], [{"mesh": 0, "camK": K, "R": R, "t": t}], H, W)[0]
    rs = np.random.RandomState(seed)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    wall = (1.1 + 0.05 * np.sin(jj / 31.0) * np.cos(ii / 23.0)).astype(np.float32)
    d = np.where(obj > 0, obj + rs.normal(scale=0.0005, size=obj.shape).astype(np.float32), wall).astype(np.float32)
    d[rs.rand(H, W) < 0.03] = 0
    return d, obj > 0


def union_of(obj_mask, d, grow=1):
    m = obj_mask.copy()
    for _ in range(grow):
        m[1:] |= m[:-1]; m[:-1] |= m[1:]; m[:, 1:] |= m[:, :-1]; m[:, :-1] |= m[:, 1:]
    return (m & (np.nan_to_num(d) > 0.2)).astype(np.uint8)


def perturbed(k, deg=3.0, mm=(6.0, -4.0, 10.0)):
    R, t = true_pose(k)
    return D.rot(1, deg) @ D.rot(0, -deg / 2) @ R, t + np.asarray(mm)


@pytest.fixture(scope="module")
def frames(ctx, mesh):
    return [frame(ctx, mesh, k, 100 + k) for k in range(4)]


def jobs_for(frames, n, seed=0, grow=1):
    rs = np.random.RandomState(seed)
    out = []
    for q in range(n):
        k = q % len(frames)
        d, om = frames[k]
        R, t = perturbed(k, deg=rs.uniform(-4, 4), mm=rs.uniform(-10, 10, 3))
        out.append({"mesh": 0, "image": k, "camK": K, "R": R, "t": t, "union_mask": union_of(om, d, grow)})
    return out


def host_chain(ctx, mesh, depths, jobs):
    from pix2pose_amd import runtime
    ins = runtime.icp_inputs_batch(ctx, [mesh], depths, jobs)
    out = []
    for jb, rec in zip(jobs, ins):
        if rec["status"] != 0:
            out.append((rec["status"], None, None, None))
            continue
        r = I.icp(rec["src"], rec["tgt"])
        if r["status"] != 0:
            out.append((r["status"], None, None, None))
            continue
        R, t = I.refined_pose(r["pose"], jb["R"], rec["t_adjusted"])
        out.append((0, R, t, r))
    return out


def test_refine_matches_the_host_chain_and_its_own_score(ctx, mesh, frames):
    from pix2pose_amd import runtime
    depths = [f[0] for f in frames]
    jobs = jobs_for(frames, 8)
    got, masks = runtime.refine_depth_batch(ctx, [mesh], depths, jobs, inlier_masks=True)
    want = host_chain(ctx, mesh, depths, jobs)
    for g, (st, R, t, r), jb in zip(got, want, jobs):
        assert g["status"] == st == 0
        assert g["iterations"][:2] == r["iterations"][:2] and g["pairs"][:2] == r["pairs"][:2]
        assert np.abs(g["R"] - R).max() <= 1e-9
        assert np.abs(g["t"] - t).max() <= 1e-6
        assert np.abs(g["icp_pose"] - r["pose"]).max() <= 1e-9
    # the score is depth_score_batch's at the returned pose, bit for bit, inlier masks included
    sjobs = [dict(jb, R=g["R"], t=g["t"]) for jb, g in zip(jobs, got)]
    sc, sm = runtime.depth_score_batch(ctx, [mesh], depths, sjobs, inlier_masks=True)
    for g, s in zip(got, sc):
        assert (g["inlier_count"], g["union_count"], g["fcn"], g["ratio"]) == (s["inlier_count"], s["union"], s["fcn"], s["ratio"])
    assert np.array_equal(masks, sm)


def test_gated_statuses_pass_through(ctx, mesh, frames):
    from pix2pose_amd import _lib, runtime
    depths = [f[0].copy() for f in frames[:2]]
    d, om = frames[0]
    good = jobs_for(frames[:1], 1)[0]
    # -1: the render misses the union mask entirely (empty init_mask)
    off = dict(good, union_mask=np.pad(np.ones((10, 10), np.uint8), ((0, H - 10), (0, W - 10))))
    # -2: a bbox of 7 x 7 but only 7 init_mask pixels (a diagonal of the union mask inside the object)
    ys, xs = np.nonzero(om)
    cy, cx = int(np.median(ys)), int(np.median(xs))
    diag = np.zeros((H, W), np.uint8)
    for q in range(7):
        diag[cy + q, cx + q] = 1
    few = dict(good, union_mask=diag & (d > 0).astype(np.uint8))
    # -3: a NaN sensor pixel inside the union mask
    depths[1] = depths[0].copy()
    um = good["union_mask"].copy()
    yy, xx = np.nonzero(um)
    depths[1][yy[len(yy) // 2], xx[len(xx) // 2]] = np.nan
    nan = dict(good, image=1, union_mask=um)
    jobs = [off, few, nan, good]
    got, masks = runtime.refine_depth_batch(ctx, [mesh], depths, jobs, inlier_masks=True)
    assert [g["status"] for g in got] == [_lib.ICP_SMALL_BBOX, _lib.ICP_FEW_POINTS, _lib.ICP_NONFINITE, 0]
    for g, jb in zip(got[:3], jobs[:3]):
        assert np.array_equal(g["R"], np.asarray(jb["R"])) and np.array_equal(g["t"], np.asarray(jb["t"]))
        assert np.array_equal(g["icp_pose"], np.eye(4))
        assert (g["inlier_count"], g["union_count"], g["fcn"], g["ratio"]) == (0, 0, 0.0, 0.0)
    assert not masks[:3].any() and masks[3].any()
    assert got[3]["inlier_count"] > 0


def test_known_pose_is_recovered(ctx, mesh, frames):
    from pix2pose_amd import runtime
    depths = [f[0] for f in frames]
    jobs = jobs_for(frames, 4, seed=3, grow=0)
    got = runtime.refine_depth_batch(ctx, [mesh], depths, jobs)
    want = host_chain(ctx, mesh, depths, jobs)
    for k, (g, w, jb) in enumerate(zip(got, want, jobs)):
        R0, t0 = true_pose(k)
        assert g["status"] == 0
        start = (I.rotation_error_deg(jb["R"], R0), np.linalg.norm(g["t_adjusted"] - t0))     # where the ICP starts
        eg = (I.rotation_error_deg(g["R"], R0), np.linalg.norm(g["t"] - t0))
        ew = (I.rotation_error_deg(w[1], R0), np.linalg.norm(w[2] - t0))
        assert eg[0] <= ew[0] + 0.01 and eg[1] <= ew[1] + 0.05
        assert eg[0] < start[0] and eg[1] < start[1], (k, start, eg)
        assert eg[1] < np.linalg.norm(jb["t"] - t0), k                                          # and than the job's own t


def test_256_jobs_over_4_frames_alone_and_in_a_batch(ctx, mesh, frames):
    from pix2pose_amd import runtime
    depths = [f[0] for f in frames]
    jobs = jobs_for(frames, 256, seed=9)
    allr = runtime.refine_depth_batch(ctx, [mesh], depths, jobs)
    assert all(g["status"] == 0 for g in allr)
    for k in (0, 5, 130, 255):
        alone = runtime.refine_depth_batch(ctx, [mesh], depths, [jobs[k]])[0]
        for key in ("R", "t", "icp_pose", "iterations", "pairs", "fval_min", "inlier_count", "fcn"):
            assert np.array_equal(np.asarray(alone[key]), np.asarray(allr[k][key])), (k, key)
    want = host_chain(ctx, mesh, depths, [jobs[17]])[0]
    assert np.abs(allr[17]["R"] - want[1]).max() <= 1e-9 and np.abs(allr[17]["t"] - want[2]).max() <= 1e-6


def test_argument_errors(ctx, mesh, frames):
    from pix2pose_amd import _lib, runtime
    depths = [frames[0][0]]
    jobs = jobs_for(frames[:1], 1)
    for prm in (dict(num_levels=0), dict(max_iterations=0), dict(rejection_scale=float("nan"))):
        with pytest.raises(_lib.P2PError):
            runtime.refine_depth_batch(ctx, [mesh], depths, jobs, **prm)
    with pytest.raises(_lib.P2PError):
        runtime.refine_depth_batch(ctx, [mesh], depths, [dict(jobs[0], mesh=3)])
    assert runtime.refine_depth_batch(ctx, [mesh], depths, []) == []
