"""Device memory of the depth path over repeated calls: every entry point of csrc/depth.hip, normals.hip, icp.hip and rgbd.hip frees
what it allocates, on success and on an error return after its allocations (the ICP-inputs capacity error, a refinement whose ICP check
fails after the ICP-inputs stage).  32 jobs at 640 x 480 per call, so a leaked image-sized buffer of any call costs more than the
16 MB bound over ten rounds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 480, 640
K = D.K_640
N_JOBS = 32
BOUND = 16 << 20


def true_pose(k):
    R = D.rot(0, 20 + 7 * k) @ D.rot(1, -25 + 11 * k) @ D.rot(2, 5 * k)
    t = np.array([-40.0 + 25 * k, 20.0 - 10 * k, 650.0 + 30 * k])
    return R, t


@pytest.fixture(scope="module")
def scene():
    from pix2pose_amd.runtime import Context, Mesh, render_depth_batch
    ctx = Context(0, max_batch=8)
    mesh = Mesh(ctx, *D.l_mesh(8))
    rs = np.random.RandomState(5)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    wall = (1.1 + 0.05 * np.sin(jj / 31.0) * np.cos(ii / 23.0)).astype(np.float32)
    depths, sils = [], []
    for k in range(4):
        R, t = true_pose(k)
        obj = render_depth_batch(ctx, [mesh], [{"mesh": 0, "camK": K, "R": R, "t": t}], H, W)[0]
        depths.append(np.where(obj > 0, obj + rs.normal(scale=0.0005, size=obj.shape).astype(np.float32), wall).astype(np.float32))
        sils.append(obj > 0)
    jobs = []
    for j in range(N_JOBS):
        R, t = true_pose(j % 4)
        jobs.append({"image": j % 4, "mesh": 0, "camK": K, "R": D.rot(1, rs.uniform(-3, 3)) @ R, "t": t + rs.uniform(-8, 8, 3),
                     "union_mask": sils[j % 4]})
    # a job whose union is a 7 x 7 block inside frame 0's silhouette: 10..63 source points, too few for 8 pyramid levels
    ys, xs = np.nonzero(sils[0])
    cy, cx = int(np.median(ys)), int(np.median(xs))
    small = np.zeros((H, W), bool)
    small[cy - 3:cy + 4, cx - 3:cx + 4] = True
    assert (small <= sils[0]).all()
    bad = jobs[:N_JOBS - 1] + [dict(jobs[0], union_mask=small)]
    yield ctx, mesh, depths, sils, jobs, bad
    mesh.close()
    ctx.close()


def one_round(scene):
    from pix2pose_amd import _lib, runtime
    ctx, mesh, depths, sils, jobs, bad = scene
    runtime.render_depth_batch(ctx, [mesh], jobs, H, W)
    runtime.depth_score_batch(ctx, [mesh], depths, jobs, inlier_masks=True)
    runtime.depth_points_batch(ctx, depths, [K] * len(depths))
    # p2p_icp_inputs_batch with a source capacity one point short (P2P_ERR_CAPACITY after the whole stage), then with enough
    keep = []
    arr = runtime._depth_jobs(jobs, keep)
    mh = (C.c_void_p * 1)(mesh.handle.value)
    dp = (C.c_void_p * len(depths))(*[d.ctypes.data for d in depths])
    res = (_lib.IcpInput * N_JOBS)()
    L = _lib.lib()
    assert L.p2p_icp_inputs_batch(ctx.handle, mh, 1, dp, len(depths), arr, N_JOBS, H, W, res, None, 0, None, 0) == 0
    n_src = sum(r.n_src for r in res)
    n_tgt = sum(r.n_tgt for r in res)
    src = np.zeros((n_src, 6), np.float32)
    tgt = np.zeros((n_tgt, 6), np.float32)
    rc = L.p2p_icp_inputs_batch(ctx.handle, mh, 1, dp, len(depths), arr, N_JOBS, H, W, res, src.ctypes.data, n_src - 1, tgt.ctypes.data,
                                n_tgt)
    assert rc == _lib.ERR_CAPACITY
    rc = L.p2p_icp_inputs_batch(ctx.handle, mh, 1, dp, len(depths), arr, N_JOBS, H, W, res, src.ctypes.data, n_src, tgt.ctypes.data, n_tgt)
    assert rc == 0
    inputs = [{"status": r.status, "src": src[r.src_offset:r.src_offset + r.n_src], "tgt": tgt[r.tgt_offset:r.tgt_offset + r.n_tgt]}
              for r in res]
    assert sum(r["status"] == 0 for r in runtime.icp_batch(ctx, inputs)) > N_JOBS // 2
    runtime.refine_depth_batch(ctx, [mesh], depths, jobs, inlier_masks=True)
    with pytest.raises(_lib.P2PError, match="pyramid levels"):
        runtime.refine_depth_batch(ctx, [mesh], depths, bad, num_levels=8)
    # a chunk on the device, created and destroyed every round
    rg = runtime.Rgbd(ctx)
    rg.load([np.full((H, W, 3), 100, np.uint8)] * 4, [d * 1000 for d in depths], [1.0] * 4, np.array(sils), [0, 1, 2, 3])
    recs, cnt = rg.refine([mesh], [dict(j, union_mask=None) for j in jobs], [j % 4 for j in range(N_JOBS)])
    assert (cnt > 30).all()
    images = [{"targets": [1], "inst_counts": [1], "rois": [{"obj": 1, "score": 0.9, "valid": True, "mask": i, "cands": [(1, i)]}]}
              for i in range(4)]
    roi_used, inst_pred = np.zeros(4, np.int32), np.zeros(4, np.int32)
    rg.resolve(0, images, roi_used, inst_pred)
    rg.close()


def test_small_job_reaches_the_icp_check(scene):
    from pix2pose_amd import runtime
    ctx, mesh, depths, sils, jobs, bad = scene
    r = runtime.icp_inputs_batch(ctx, [mesh], depths, bad[-1:])[0]
    assert r["status"] == 0 and 10 <= len(r["src"]) <= 63


def test_repeated_calls_do_not_grow_device_memory(scene):
    import torch
    free = []
    for _ in range(2):
        one_round(scene)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print("free device memory after the two warm-up rounds: %d, %d bytes" % tuple(free))
    for _ in range(10):
        one_round(scene)
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    print("after ten more rounds: %d bytes (drop %.1f MB)" % (after, (free[-1] - after) / 2**20))
    assert free[-1] - after <= BOUND, (free, after)
