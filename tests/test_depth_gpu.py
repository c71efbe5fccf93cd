"""GPU tests of the depth path (csrc/depth.hip): the mesh z-buffer and the depth score against the float64 restatement
(tests/depth_ref.py), culling on an outward mesh, batch independence and argument checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 480, 640


@pytest.fixture(scope="module")
def ctx():
    from pix2pose_amd.runtime import Context
    c = Context(0, max_batch=8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lmesh(ctx):
    from pix2pose_amd.runtime import Mesh
    v, t = D.l_mesh(8)
    return v, t, Mesh(ctx, v, t)


def _poses(n, seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        R = D.rot(0, rs.uniform(-180, 180)) @ D.rot(1, rs.uniform(-180, 180)) @ D.rot(2, rs.uniform(-180, 180))
        z = rs.uniform(0.35, 1.2)
        t = np.array([rs.uniform(-0.15, 0.15) * z, rs.uniform(-0.1, 0.1) * z, z]) * 1000.0      # mm
        out.append((R, t))
    return out


def _job(R, t, mesh=0, image=0, mask=None, K=D.K_640):
    j = {"mesh": mesh, "image": image, "camK": K, "R": R, "t": t}
    if mask is not None:
        j["union_mask"] = mask
    return j


def _compare(dg, dr, margin):
    both = (dg > 0) & (dr > 0)
    rel = np.abs(dg[both].astype(np.float64) - dr[both]) / dr[both]
    flip = (dg > 0) != (dr > 0)
    assert rel.max(initial=0) <= 1e-6, rel.max()
    assert not np.any(flip & ~margin), "coverage differs away from an edge at %s" % (np.argwhere(flip & ~margin)[:5],)
    return int(flip.sum())


def test_render_depth_equals_restatement(ctx, lmesh):
    from pix2pose_amd.runtime import render_depth_batch
    v, t, m = lmesh
    poses = _poses(8, 1)
    poses += [(D.rot(1, 15), np.array([0.0, 0.0, 30.0])),         # straddles the near plane
              (D.rot(0, 40), np.array([250.0, 100.0, 400.0])),    # partly outside the image
              (D.rot(2, 5), np.array([3000.0, 0.0, 300.0])),      # entirely outside
              (np.eye(3), np.array([0.0, 0.0, -500.0])),          # behind the camera
              (D.rot(1, 170), np.array([2e4, -1e4, 6.5e5])),      # t_z / 1000 > 100: render_obj's unit quirk
              (D.rot(0, 30), np.array([0.0, 0.0, 45.0]))]         # 10 mm in front of the camera: huge triangles
    dg = render_depth_batch(ctx, [m], [_job(R, tt) for R, tt in poses], H, W)
    flips = 0
    for k, (R, tt) in enumerate(poses):
        dr, margin = D.render_depth(v, t, D.K_640, R, tt, H, W, with_margin=True)
        flips += _compare(dg[k], dr, margin)
        assert np.all((dg[k] == 0) | ((dg[k] >= 0.01) & (dg[k] <= 10)))
    assert (dg[:8] > 0).sum(axis=(1, 2)).min() > 500
    print("coverage differences at edge-grazing centres: %d" % flips)


def test_render_culls_back_faces_of_an_outward_mesh(ctx):
    from pix2pose_amd.runtime import Mesh, render_depth_batch
    v, t = D.box_mesh([-50, -50, -50], [50, 50, 50], 3)
    out_m, in_m = Mesh(ctx, v, t), Mesh(ctx, v, t[:, ::-1])
    d = render_depth_batch(ctx, [out_m, in_m], [_job(np.eye(3), [0, 0, 500], 0), _job(np.eye(3), [0, 0, 500], 1)], H, W)
    j, i = int(D.K_640[1, 2]), int(D.K_640[0, 2])
    assert abs(d[0, j, i] - 0.45) < 1e-6 and abs(d[1, j, i] - 0.55) < 1e-6
    assert np.array_equal(d[0] > 0, d[1] > 0)


def _scene(ctx, lmesh, n_img=4, per_img=8, seed=3):
    """Sensor depth images rendered from ground-truth poses (noise, holes); jobs at perturbed poses with box masks."""
    from pix2pose_amd.runtime import render_depth_batch
    v, t, m = lmesh
    rs = np.random.RandomState(seed)
    poses = _poses(n_img * per_img, seed)
    gt = render_depth_batch(ctx, [m], [_job(R, tt) for R, tt in poses], H, W)
    depths = []
    for i in range(n_img):
        img = np.zeros((H, W), np.float32)
        for k in range(per_img):
            g = gt[i * per_img + k]
            img = np.where((g > 0) & ((img == 0) | (g < img)), g, img)
        img = img + rs.normal(0, 0.003, img.shape).astype(np.float32) * (img > 0)
        img[rs.rand(H, W) < 0.05] = 0
        depths.append(img.astype(np.float32))
    jobs = []
    for k, (R, tt) in enumerate(poses):
        Rp = R @ D.rot(rs.randint(3), rs.uniform(-8, 8))
        tp = tt + rs.uniform(-15, 15, 3)
        jj, ii = np.nonzero(gt[k] > 0)
        mask = np.zeros((H, W), np.uint8)
        if len(jj):
            mask[jj.min():jj.max() + 1, ii.min():ii.max() + 1] = 1
        jobs.append(_job(Rp, tp, image=k // per_img, mask=mask))
    return depths, jobs


def test_depth_score_equals_restatement(ctx, lmesh):
    from pix2pose_amd.runtime import depth_score_batch, render_depth_batch
    v, t, m = lmesh
    depths, jobs = _scene(ctx, lmesh)
    res, inl = depth_score_batch(ctx, [m], depths, jobs, inlier_masks=True)
    ref_depth = render_depth_batch(ctx, [m], jobs, H, W)
    n_edge = 0
    for k, j in enumerate(jobs):
        dr, margin = D.render_depth(v, t, D.K_640, j["R"], j["t"], H, W, with_margin=True)
        n_edge += _compare(ref_depth[k], dr, margin)
        # the score from the GPU's own rendering is exact up to summation order ...
        s, im = D.depth_score(ref_depth[k], depths[j["image"]], j["union_mask"])
        assert res[k]["union"] == s["union"] and res[k]["inlier_count"] == s["inlier_count"], (k, res[k], s)
        assert abs(res[k]["fcn"] - s["fcn"]) <= 1e-12 * max(1.0, s["fcn"])
        assert res[k]["ratio"] == s["ratio"]
        assert np.array_equal(inl[k], im)
        # ... and from the restatement's rendering it differs only where coverage grazes an edge
        s2, _ = D.depth_score(dr, depths[j["image"]], j["union_mask"])
        assert abs(res[k]["inlier_count"] - s2["inlier_count"]) <= int(margin.sum())
    assert sum(r["inlier_count"] for r in res) > 1000


def test_batch_results_are_bit_identical_to_single_jobs(ctx, lmesh):
    from pix2pose_amd.runtime import depth_score_batch, render_depth_batch
    _, _, m = lmesh
    depths, jobs = _scene(ctx, lmesh, seed=5)
    assert len(jobs) == 32
    dall = render_depth_batch(ctx, [m], jobs, H, W)
    sall = depth_score_batch(ctx, [m], depths, jobs)
    for k, j in enumerate(jobs):
        one = render_depth_batch(ctx, [m], [j], H, W)[0]
        assert np.array_equal(one.view(np.uint32), dall[k].view(np.uint32))
        s1 = depth_score_batch(ctx, [m], [depths[j["image"]]], [dict(j, image=0)])[0]
        assert s1 == sall[k]
    # rendering is order-independent: the same mesh with its triangles reversed draws the same bits
    v, t, _ = lmesh
    from pix2pose_amd.runtime import Mesh
    rev = Mesh(ctx, v, t[::-1].copy())
    drev = render_depth_batch(ctx, [rev], jobs[:4], H, W)
    assert np.array_equal(drev.view(np.uint32), dall[:4].view(np.uint32))


def test_mesh_from_ply_renders_like_the_arrays(ctx, lmesh, tmp_path):
    from pix2pose_amd.runtime import Mesh, render_depth_batch
    v, t, m = lmesh
    fn = str(tmp_path / "obj_000001.ply")
    hdr = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" \
          "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(t))
    fr = np.zeros(len(t), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    fr["n"], fr["v"] = 3, t
    open(fn, "wb").write(hdr.encode() + v.astype("<f4").tobytes() + fr.tobytes())
    mp = Mesh.from_ply(ctx, fn)
    jobs = [_job(R, tt) for R, tt in _poses(3, 9)]
    assert np.array_equal(render_depth_batch(ctx, [mp], jobs, H, W), render_depth_batch(ctx, [m], jobs, H, W))


def test_bad_arguments_are_errors_not_faults(ctx, lmesh):
    from pix2pose_amd import _lib
    from pix2pose_amd.runtime import Mesh, depth_score_batch, render_depth_batch
    _, _, m = lmesh
    with pytest.raises(_lib.P2PError):
        Mesh(ctx, np.zeros((3, 3)), [[0, 1, 3]])                  # vertex index out of range
    with pytest.raises(_lib.P2PError):
        render_depth_batch(ctx, [m], [_job(np.eye(3), [0, 0, 500], mesh=1)], H, W)
    mask = np.ones((H, W), np.uint8)
    with pytest.raises(_lib.P2PError):
        depth_score_batch(ctx, [m], [np.zeros((H, W), np.float32)], [_job(np.eye(3), [0, 0, 500], image=2, mask=mask)])
    empty = Mesh(ctx, np.zeros((3, 3)), np.zeros((0, 3), np.int32))
    assert not render_depth_batch(ctx, [empty], [_job(np.eye(3), [0, 0, 500])], H, W).any()


def test_tie_rule_on_pixel_centre_vertices_matches_exactly(ctx):
    """Every edge of this mesh runs through pixel centres (tests/depth_ref.py: pixel_grid_mesh): coverage must equal the
    restatement with no edge allowance at all, and the depth is exactly 1 m."""
    from pix2pose_amd.runtime import Mesh, render_depth_batch
    v, t = D.pixel_grid_mesh()
    d = render_depth_batch(ctx, [Mesh(ctx, v, t)], [_job(np.eye(3), [0, 0, 1000], K=D.GRID_K)], H, W)[0]
    dr, counts = D.render_depth(v, t, D.GRID_K, np.eye(3), [0, 0, 1000], H, W, with_counts=True)
    assert counts.max() == 1 and counts.sum() == 64 * 64
    assert np.array_equal(d > 0, counts > 0) and np.all(d[d > 0] == 1.0)


def test_large_and_near_triangles(ctx):
    """A 2-triangle plane filling the whole image, and a mesh 1 cm in front of the camera: the large-triangle route gives the
    restatement's depth (the per-triangle route would walk the whole image in one thread)."""
    from pix2pose_amd.runtime import Mesh, render_depth_batch
    verts = np.array([[-2000, -2000, 0], [2000, -2000, 0], [2000, 2000, 0], [-2000, 2000, 0]], np.float64)
    tris = np.array([[0, 2, 1], [0, 3, 2]])
    big = Mesh(ctx, verts, tris)
    v, t, = D.l_mesh(2)
    lm = Mesh(ctx, v, t)
    jobs = [_job(D.rot(0, 10), [0, 0, 800], mesh=0), _job(D.rot(1, 25), [5, 0, 35], mesh=1), _job(D.rot(0, 200), [0, 0, 40], mesh=1)]
    dg = render_depth_batch(ctx, [big, lm], jobs, H, W)
    for k, (vv, tt) in enumerate([(verts, tris), (v, t), (v, t)]):
        dr, margin = D.render_depth(vv, tt, D.K_640, jobs[k]["R"], jobs[k]["t"], H, W, with_margin=True)
        _compare(dg[k], dr, margin)
    assert (dg[0] > 0).sum() > 0.9 * H * W and (dg[1] > 0).sum() > 0.3 * H * W
