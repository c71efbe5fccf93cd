"""GPU tests of the depth path (csrc/depth.hip): the mesh z-buffer and the depth score against the float64 restatement
(tests/depth_ref.py) and, on small images, the ray-cast oracle: culling on an outward mesh, image sizes and cameras, both raster
routes, the clip and quirk boundaries at their exact values, the score's edges, batch independence and argument checks."""
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


# --- sizes, cameras, routes, boundaries, score edges and batch shapes (the restatement and the ray-cast oracle as references) ---

def _ref(verts, tris, job, H, W):
    return D.render_depth(verts, tris, job["camK"], job["R"], job["t"], H, W, with_margin=True)


def _shapes():
    """The cameras of depth_ref.CAMERAS at their sizes, plus a single row and a single column of the 640 x 480 camera."""
    K0 = D.CAMERAS[0][0]
    return list(D.CAMERAS) + [(K0, 1, 640), (K0, 480, 1)]


def test_image_sizes_and_cameras(ctx, lmesh):
    """Skew of both signs, fx != fy, off-centre principal points, H * W not a multiple of 256, 1 x W and H x 1: the kernels
    render the asymmetric L mesh as the restatement does (and as the ray caster does on the small image), and score it as
    the restatement scores the GPU's rendering, which runs the tail of the score kernel's strided loop."""
    from pix2pose_amd.runtime import depth_score_batch, render_depth_batch
    v, t, m = lmesh
    rs = np.random.RandomState(21)
    n_cov = 0
    for K, h, w in _shapes():
        jobs = []
        for k in range(4):
            R, tt = D.random_pose(rs, K, max(h, 2), max(w, 2), 0.35, 1.0)
            if h == 1 or w == 1:                 # put the object's origin on the single row / column
                R, tt = D.random_pose(rs, K, 480, 640, 0.35, 1.0)
                p = np.linalg.solve(K, [0.5 if w == 1 else rs.uniform(100, 540), 0.5 if h == 1 else rs.uniform(80, 400), 1.0])
                tt = p / p[2] * tt[2]
            mask = (rs.rand(h, w) < 0.7).astype(np.uint8)
            jobs.append(dict(_job(R, tt, K=K, image=k % 2), union_mask=mask))
        dg = render_depth_batch(ctx, [m], jobs, h, w)
        for k, j in enumerate(jobs):
            dr, margin = _ref(v, t, j, h, w)
            _compare(dg[k], dr, margin)
            if h * w < 4000:
                rc, m2 = D.raycast_depth(v, t, K, j["R"], j["t"], h, w)
                _compare(dg[k], rc, margin | m2)
            n_cov += int((dg[k] > 0).sum())
        # sensor images: the rendering plus noise around the inlier threshold, and holes
        depths = []
        for i in range(2):
            base = np.where(dg[i] > 0, dg[i], np.float32(0.8))
            depths.append((base + rs.uniform(-0.03, 0.03, (h, w))).astype(np.float32))
        res, inl = depth_score_batch(ctx, [m], depths, jobs, inlier_masks=True)
        for k, j in enumerate(jobs):
            s, im = D.depth_score(dg[k], depths[j["image"]], j["union_mask"])
            assert (res[k]["inlier_count"], res[k]["union"]) == (s["inlier_count"], s["union"]), (h, w, k)
            assert abs(res[k]["fcn"] - s["fcn"]) <= 1e-12 * max(1.0, s["fcn"]) and res[k]["ratio"] == s["ratio"]
            assert np.array_equal(inl[k], im)
    assert n_cov > 50000


def _plane(n, side_mm):
    """A flat n x n-quad square of the given side at z = 0, its front (+z normal by winding) towards -z, i.e. seen by a camera on -z."""
    g = np.linspace(-side_mm / 2, side_mm / 2, n + 1)
    verts = np.array([(x, y, 0.0) for y in g for x in g])
    tris = []
    for a in range(n):
        for b in range(n):
            q = [a * (n + 1) + b, a * (n + 1) + b + 1, (a + 1) * (n + 1) + b + 1, (a + 1) * (n + 1) + b]
            tris += [(q[0], q[2], q[1]), (q[0], q[3], q[2])]
    return verts, np.array(tris)


def _route2_count(verts, tris, job, H, W):
    """Host copy of the kernel's route choice: drawn (front-facing, not rejected) triangles whose clamped box holds > 1024 centres."""
    u, v, z = D.project(verts, job["camK"], job["R"], job["t"])
    n = 0
    for f in tris:
        uu, vv = u[f], v[f]
        if not np.all(z[f] >= D.CLIP_NEAR):
            continue
        if not (uu[1] - uu[0]) * (vv[2] - vv[0]) - (uu[2] - uu[0]) * (vv[1] - vv[0]) < 0:
            continue
        i0, i1 = max(0, np.ceil(uu.min() - 0.5)), min(W - 1, np.floor(uu.max() - 0.5))
        j0, j1 = max(0, np.ceil(vv.min() - 0.5)), min(H - 1, np.floor(vv.max() - 0.5))
        n += (i1 >= i0 and j1 >= j0 and (i1 - i0 + 1) * (j1 - j0 + 1) > 1024)
    return n


def test_more_than_1024_large_triangles_in_one_call(ctx):
    """A 20 x 20-quad plane close to the camera in three jobs: every triangle's box holds > 1024 centres, so route 2 gets more
    list entries than it has workgroups and must stride over the list."""
    from pix2pose_amd.runtime import Mesh, render_depth_batch
    h, w = 960, 1280
    K = np.array([[500.0, 0.0, 640.0], [0.0, 500.0, 480.0], [0.0, 0.0, 1.0]])
    verts, tris = _plane(20, 800.0)
    m = Mesh(ctx, verts, tris)
    jobs = [_job(np.eye(3), [0, 0, 500], K=K), _job(D.rot(0, 20) @ D.rot(1, -15), [20, -30, 520], K=K),
            _job(D.rot(2, 40), [-50, 10, 480], K=K)]
    n2 = sum(_route2_count(verts, tris, j, h, w) for j in jobs)
    assert n2 > 1024, n2
    dg = render_depth_batch(ctx, [m], jobs, h, w)
    for k, j in enumerate(jobs):
        dr, margin = _ref(verts, tris, j, h, w)
        _compare(dg[k], dr, margin)
        assert (dg[k] > 0).sum() > 0.3 * h * w
    print("route-2 entries: %d" % n2)


def test_small_and_large_triangles_overlapping(ctx):
    """A fine box (route 1) pierced by a coarse tilted plane (route 2), so each is in front of the other on some pixels: the
    result is the restatement's, and the bits do not change with the triangle order reversed or the two meshes' triangles and
    the jobs swapped."""
    from pix2pose_amd.runtime import Mesh, render_depth_batch
    fv, ft = D.box_mesh([-60, -45, -40], [60, 45, 40], 12)
    cv = np.array([[-400, -300, 0], [400, -300, 0], [400, 300, 0], [-400, 300, 0]], np.float64)
    cv = cv @ D.rot(1, 55).T
    ct = np.array([[0, 2, 1], [0, 3, 2]])
    fine_first = (np.concatenate([fv, cv]), np.concatenate([ft, ct + len(fv)]))
    coarse_first = (np.concatenate([cv, fv]), np.concatenate([ct, ft + len(cv)]))
    ma, mb = Mesh(ctx, *fine_first), Mesh(ctx, *coarse_first)
    mr = Mesh(ctx, fine_first[0], fine_first[1][::-1].copy())
    poses = [(np.eye(3), [0, 0, 450]), (D.rot(0, 15) @ D.rot(2, 30), [10, -5, 420]), (D.rot(2, 90), [0, 0, 450])]
    jobs_a = [_job(R, tt, mesh=0) for R, tt in poses]
    da = render_depth_batch(ctx, [ma, mb, mr], jobs_a, H, W)
    for k, j in enumerate(jobs_a):
        dr, margin = _ref(*fine_first, j, H, W)
        _compare(da[k], dr, margin)
        # both surfaces win somewhere: the box alone and the plane alone each give the nearest depth on > 1000 pixels
        db_, _ = _ref(fv, ft, j, H, W)
        dc_, _ = _ref(cv, ct, j, H, W)
        both = (db_ > 0) & (dc_ > 0)
        assert (both & (db_ < dc_)).sum() > 1000 and (both & (dc_ < db_)).sum() > 1000
    for mesh in (1, 2):
        jobs = [_job(R, tt, mesh=mesh) for R, tt in poses][::-1]
        d = render_depth_batch(ctx, [ma, mb, mr], jobs, H, W)[::-1]
        assert np.array_equal(d.view(np.uint32), da.view(np.uint32)), mesh


def _first_above(x, limit, scale):
    """The smallest double t >= x with t / scale > limit (t / scale rounds, so the next double above limit * scale may not do)."""
    t = x
    while not t / scale > limit:
        t = np.nextafter(t, np.inf)
    return float(t)


def _last_below(x, limit, scale):
    t = x
    while not t / scale < limit:
        t = np.nextafter(t, -np.inf)
    return float(t)


def test_near_plane_boundary_at_its_exact_value(ctx):
    """A vertex exactly at z_c = 0.01 m keeps its triangle; one a rounding below rejects it.  t_z = 10 mm divides to exactly
    the double 0.01 (division is correctly rounded, so 10 / 1000 is the double nearest 0.01, the same as the constant), and
    the vertex is at the model origin with R = I, so z_c = 0 + 0 + 0 + 0.01 exactly."""
    from pix2pose_amd.runtime import Mesh, render_depth_batch
    verts = np.array([[0, 0, 0], [60, -40, 60], [-50, -40, 60], [0, 70, 60]], np.float64)
    tris = np.array([[0, 1, 2], [0, 2, 1], [0, 2, 3], [0, 3, 2], [0, 3, 1], [0, 1, 3]])      # both windings: one of each drawn
    m = Mesh(ctx, verts, tris)
    assert 10.0 / 1000.0 == D.CLIP_NEAR
    below = _last_below(10.0, D.CLIP_NEAR, 1000.0)
    jobs = [_job(np.eye(3), [0, 0, 10.0]), _job(np.eye(3), [0, 0, below])]
    dg = render_depth_batch(ctx, [m], jobs, H, W)
    for k, j in enumerate(jobs):
        dr, margin = _ref(verts, tris, j, H, W)
        _compare(dg[k], dr, margin)
    assert (dg[0] > 0).sum() > 10000
    assert not dg[1].any()


def test_far_clip_at_its_exact_value(ctx):
    """A 2 x 2-quad square at z = 10 m whose vertices project onto pixel centres (x, y = 0 or +-2.5 m: float32(2500) * float32(0.001)
    is exactly 2.5, 2.5 / 10 = 0.25 exactly, u = 64 * 0.25 + 320.5).  At the pixel of its centre vertex the owning triangle's edge
    functions are exactly (A, 0, 0), so 1/z = 0.1 and d = 1 / 0.1 = 10.0 exactly: drawn.  With t_z one rounding beyond 10 m, dropped."""
    from pix2pose_amd.runtime import Mesh, render_depth_batch
    g = [-2500.0, 0.0, 2500.0]
    verts = np.array([(x, y, 0.0) for y in g for x in g])
    assert np.array_equal(D.mesh_metres(verts)[:, :2], np.array(verts[:, :2]) / 1000)
    tris = []
    for a in range(2):
        for b in range(2):
            q = [a * 3 + b, a * 3 + b + 1, (a + 1) * 3 + b + 1, (a + 1) * 3 + b]
            tris += [(q[0], q[3], q[1]), (q[1], q[3], q[2])]
    tris = np.array(tris)
    m = Mesh(ctx, verts, tris)
    assert 1.0 / ((1.0 / 1.0) / 10.0 + (0.0 / 1.0) / 10.0 + (0.0 / 1.0) / 10.0) == D.CLIP_FAR
    beyond = _first_above(10000.0, D.CLIP_FAR, 1000.0)
    jobs = [_job(np.eye(3), [0, 0, 10000.0], K=D.GRID_K), _job(np.eye(3), [0, 0, beyond], K=D.GRID_K)]
    dg = render_depth_batch(ctx, [m], jobs, H, W)
    for k, j in enumerate(jobs):
        dr, margin = _ref(verts, tris, j, H, W)
        _compare(dg[k], dr, margin)
        assert np.array_equal(dg[k] > 0, dr > 0)            # no edge allowance: same rule, same arithmetic
    assert dg[0][240, 320] == np.float32(10.0)
    assert dg[1][240, 320] == 0 and not (dg[1] > 10).any()


def test_unit_quirk_at_its_exact_value(ctx, lmesh):
    """render_obj divides t once more only when t_z / 1000 > 100: t_z = 100000 mm is exactly 100 m (no quirk, beyond the far
    plane: nothing drawn); the smallest t_z with t_z / 1000 > 100, searched (the next double above 100000 may still divide to
    exactly 100.0), is drawn at 0.1 m."""
    from pix2pose_amd.runtime import render_depth_batch
    v, t, m = lmesh
    first = _first_above(100000.0, 100.0, 1000.0)
    assert first > 100000.0 and 100000.0 / 1000.0 == 100.0
    jobs = [_job(D.rot(0, 30), [0, 0, 100000.0]), _job(D.rot(0, 30), [0, 0, first])]
    dg = render_depth_batch(ctx, [m], jobs, H, W)
    assert not dg[0].any()
    dr, margin = _ref(v, t, jobs[1], H, W)
    _compare(dg[1], dr, margin)
    assert (dg[1] > 0).sum() > 10000 and abs(np.median(dg[1][dg[1] > 0]) - 0.1) < 0.03


def _raw_score(ctx, meshes, depths, jobs, masks, inlier_masks=False):
    """p2p_depth_score_batch with the union masks passed as given (any byte values), not normalised by the binding."""
    import ctypes as C
    from pix2pose_amd import _lib
    from pix2pose_amd.runtime import _depth_jobs
    keep = []
    arr = _depth_jobs(jobs, keep)
    masks = [np.ascontiguousarray(mm, dtype=np.uint8) for mm in masks]
    for k, mm in enumerate(masks):
        arr[k].union_mask = mm.ctypes.data
    depths = [np.ascontiguousarray(d, dtype=np.float32) for d in depths]
    h, w = depths[0].shape
    mh = (C.c_void_p * len(meshes))(*[x.handle.value for x in meshes])
    dp = (C.c_void_p * len(depths))(*[d.ctypes.data for d in depths])
    res = (_lib.DepthScore * len(jobs))()
    out = np.zeros((len(jobs), h, w), np.uint8) if inlier_masks else None
    _lib.check(_lib.lib().p2p_depth_score_batch(ctx.handle, mh, len(meshes), dp, len(depths), arr, len(jobs), h, w, res,
                                                out.ctypes.data if out is not None else None), "p2p_depth_score_batch")
    recs = [(r.inlier_count, r.union_count, r.fcn, r.ratio) for r in res]
    return (recs, out) if inlier_masks else recs


def test_score_edges(ctx, lmesh):
    """Empty union; union masks of 1s, 255s, other non-zero bytes, bools and int64; inlier masks on and off; every union pixel
    an inlier; six images named out of order with some unused; fcn against math.fsum."""
    import math
    from pix2pose_amd.runtime import depth_score_batch, render_depth_batch
    v, t, m = lmesh
    rs = np.random.RandomState(31)
    poses = _poses(8, 31)
    gt = render_depth_batch(ctx, [m], [_job(R, tt) for R, tt in poses], H, W)
    depths = []
    for i in range(6):
        g = gt[i]
        depths.append(np.where(g > 0, g + rs.uniform(-0.03, 0.03, g.shape), rs.uniform(0.3, 1.5, g.shape)).astype(np.float32))
    img_of = [5, 0, 3, 3, 0, 5, 1, 0]            # out of order; images 2 and 4 unused
    masks = []
    for k in range(8):
        mk = np.zeros((H, W), np.uint8)
        jj, ii = np.nonzero(gt[k] > 0)
        mk[jj.min() - 5:jj.max() + 5, ii.min() - 5:ii.max() + 5] = 1
        masks.append(mk)
    masks[7][:] = 0                                # empty union
    jobs = [_job(R, tt, image=img_of[k], mask=masks[k]) for k, (R, tt) in enumerate(poses)]
    res, inl = depth_score_batch(ctx, [m], depths, jobs, inlier_masks=True)
    assert res == depth_score_batch(ctx, [m], depths, jobs)          # inlier masks off: identical records
    assert res[7] == {"inlier_count": 0, "union": 0, "fcn": 0.0, "ratio": 0.0} and not inl[7].any()
    for k, j in enumerate(jobs[:7]):
        s, im = D.depth_score(gt[k], depths[img_of[k]], masks[k])
        assert (res[k]["inlier_count"], res[k]["union"], res[k]["ratio"]) == (s["inlier_count"], s["union"], s["ratio"])
        assert np.array_equal(inl[k], im)
        sel = masks[k] != 0
        diff = np.abs(gt[k][sel].astype(np.float64) - depths[img_of[k]][sel].astype(np.float64))
        exact = math.fsum(np.maximum(0.0, 0.02 - diff) / 0.02)
        assert abs(res[k]["fcn"] - exact) <= 1e-12 * exact, (k, res[k]["fcn"], exact)
        assert 0 < s["inlier_count"] < s["union"]
    # the same masks as other byte values and dtypes: the same records
    ref = [(r["inlier_count"], r["union"], r["fcn"], r["ratio"]) for r in res]
    other = [np.where(mk != 0, rs.randint(1, 256, mk.shape), 0) for mk in masks]
    assert _raw_score(ctx, [m], depths, jobs, [mk * 255 for mk in masks]) == ref
    recs, raw_inl = _raw_score(ctx, [m], depths, jobs, other, inlier_masks=True)
    assert recs == ref and np.array_equal(raw_inl != 0, inl) and set(np.unique(raw_inl)) <= {0, 1}
    for conv in (lambda mk: mk.astype(bool), lambda mk: mk.astype(np.int64) * 7):
        assert depth_score_batch(ctx, [m], depths, [dict(j, union_mask=conv(j["union_mask"])) for j in jobs]) == res
    # every union pixel an inlier: the mask is the rendered silhouette, the sensor the rendering plus < 0.02
    sil = (gt[0] > 0).astype(np.uint8)
    sensor = (gt[0] + rs.uniform(-0.019, 0.019, gt[0].shape)).astype(np.float32)
    r = depth_score_batch(ctx, [m], [sensor], [_job(*poses[0], mask=sil)])[0]
    assert r["inlier_count"] == r["union"] == sil.sum() and r["ratio"] == 1.0


def test_score_threshold_at_one_ulp(ctx, lmesh):
    """Sensor depths one float32 ulp either side of |dr - dt| = 0.02 from the GPU's own rendering: the counts are the reference's
    float32 rule (depth_ref.score_ref32) and the float64 restatement's, and the inlier masks equal."""
    from pix2pose_amd.runtime import depth_score_batch, render_depth_batch
    v, t, m = lmesh
    rs = np.random.RandomState(32)
    poses = _poses(4, 32)
    gt = render_depth_batch(ctx, [m], [_job(R, tt) for R, tt in poses], H, W)
    jobs, depths = [], []
    for k in range(4):
        g = gt[k]
        sign = np.where(rs.rand(H, W) < 0.5, np.float32(1), np.float32(-1))
        dt = (g + sign * np.float32(0.02)).astype(np.float32)
        step = rs.randint(-1, 2, (H, W))
        dt = np.where(step < 0, np.nextafter(dt, np.float32(0)), np.where(step > 0, np.nextafter(dt, np.float32(np.inf)), dt))
        depths.append(np.where(g > 0, dt, np.float32(0)).astype(np.float32))
        jobs.append(_job(*poses[k], image=k, mask=(g > 0).astype(np.uint8)))
    res, inl = depth_score_batch(ctx, [m], depths, jobs, inlier_masks=True)
    for k in range(4):
        s32, m32 = D.score_ref32(gt[k], depths[k], jobs[k]["union_mask"])
        s64, _ = D.depth_score(gt[k], depths[k], jobs[k]["union_mask"])
        assert res[k]["inlier_count"] == s32["inlier_count"] == s64["inlier_count"]
        assert np.array_equal(inl[k], m32)
        assert 0.2 * s32["union"] < s32["inlier_count"] < 0.8 * s32["union"]


def test_nan_sensor_pixel_rule(ctx, lmesh):
    """The NaN rule: a NaN sensor pixel inside the union counts in the union, is not an inlier and adds 0 to fcn,
    as depth_ref.depth_score states it."""
    from pix2pose_amd.runtime import depth_score_batch, render_depth_batch
    v, t, m = lmesh
    R, tt = _poses(1, 33)[0]
    g = render_depth_batch(ctx, [m], [_job(R, tt)], H, W)[0]
    sensor = (g + np.float32(0.005)).astype(np.float32)
    jj, ii = np.nonzero(g > 0)
    sensor[jj[::7], ii[::7]] = np.nan
    mask = (g > 0).astype(np.uint8)
    r, inl = depth_score_batch(ctx, [m], [sensor], [_job(R, tt, mask=mask)], inlier_masks=True)
    s, im = D.depth_score(g, sensor, mask)
    assert np.isfinite(s["fcn"]) and s["union"] == len(jj) and s["inlier_count"] == len(jj) - len(jj[::7])
    assert (r[0]["inlier_count"], r[0]["union"]) == (s["inlier_count"], s["union"]) and np.array_equal(inl[0], im)
    assert abs(r[0]["fcn"] - s["fcn"]) <= 1e-12 * s["fcn"]


def test_batch_shape_of_the_timing_tool(ctx):
    """256 jobs (tools/time_depth.py's largest batch) at 720 x 540 over meshes of 0, 1, 384 and 864 triangles, each job with its
    own camera: every job is the restatement's, 16 of them alone give the same bits, and a repeated call gives the same bits."""
    from pix2pose_amd.runtime import Mesh, render_depth_batch
    h, w = 540, 720
    one = (np.array([[-40, -40, 0], [40, -40, 0], [0, 50, 0]], np.float64), np.array([[0, 2, 1]]))
    lm = D.l_mesh(4)
    fb = D.box_mesh([-45, -35, -25], [45, 35, 25], 6)
    geo = [(np.zeros((3, 3)), np.zeros((0, 3), np.int64)), one, lm, fb]
    meshes = [Mesh(ctx, *g) for g in geo]
    rs = np.random.RandomState(41)
    K0 = D.CAMERAS[1][0]
    jobs = []
    for k in range(256):
        K = K0.copy()
        K[0, 0] *= rs.uniform(0.8, 1.2); K[1, 1] *= rs.uniform(0.8, 1.2)
        K[0, 1] = rs.uniform(-4, 4); K[0, 2] = rs.uniform(200, 520); K[1, 2] = rs.uniform(150, 390)
        R, tt = D.random_pose(rs, K, h, w, 0.4, 1.2)
        if k % 4 == 1:                # the single triangle shows its front (negative image area at R = I) within +-30 degrees
            R = D.rot(0, rs.uniform(-30, 30)) @ D.rot(1, rs.uniform(-30, 30)) @ D.rot(2, rs.uniform(-180, 180))
        jobs.append(_job(R, tt, mesh=k % 4, K=K))
    d1 = render_depth_batch(ctx, meshes, jobs, h, w)
    d2 = render_depth_batch(ctx, meshes, jobs, h, w)
    assert np.array_equal(d1.view(np.uint32), d2.view(np.uint32))
    for k, j in enumerate(jobs):
        dr, margin = _ref(*geo[j["mesh"]], j, h, w)
        _compare(d1[k], dr, margin)
    assert not d1[0::4].any() and (d1[1::4] > 0).sum(axis=(1, 2)).min() > 0
    for k in rs.choice(256, 16, replace=False):
        alone = render_depth_batch(ctx, meshes, [jobs[k]], h, w)[0]
        assert np.array_equal(alone.view(np.uint32), d1[k].view(np.uint32)), k


def test_mesh_content_edges(ctx):
    """Zero-area triangles (collinear, repeated vertex) are not drawn; a triangle given in both windings is drawn once (its
    front); vertices at +-1e4 mm render as the restatement does."""
    from pix2pose_amd.runtime import Mesh, render_depth_batch
    verts = np.array([[-60, -50, 0], [60, -50, 0], [0, 60, 0], [-30, 0, 0], [30, 0, 0], [90, 0, 0],
                      [-1e4, -1e4, 3000], [1e4, -1e4, 3000], [0, 1e4, 3000]], np.float64)
    tris = np.array([[0, 2, 1], [0, 1, 2],          # both windings
                     [3, 4, 5], [3, 5, 4],          # collinear: zero area in both windings
                     [0, 0, 2], [1, 1, 1],          # repeated vertices
                     [6, 8, 7], [6, 7, 8]])         # +-1e4 mm, behind the small one
    m = Mesh(ctx, verts, tris)
    dup = Mesh(ctx, verts, tris[:2])
    degen = Mesh(ctx, verts, tris[2:6])
    jobs = [_job(np.eye(3), [0, 0, 500], mesh=0), _job(D.rot(0, 20), [5, -10, 700], mesh=0), _job(np.eye(3), [0, 0, 500], mesh=1),
            _job(np.eye(3), [0, 0, 500], mesh=2)]
    dg = render_depth_batch(ctx, [m, dup, degen], jobs, H, W)
    geos = [(verts, tris), (verts, tris), (verts, tris[:2]), (verts, tris[2:6])]
    for k, j in enumerate(jobs):
        dr, margin = _ref(*geos[k], j, H, W)
        _compare(dg[k], dr, margin)
    _, counts = D.render_depth(verts, tris[:2], D.K_640, np.eye(3), [0, 0, 500], H, W, with_counts=True)
    assert counts.max() == 1 and counts.sum() > 1000
    assert not dg[3].any()
    assert (dg[0] > 3.0).sum() > 0.5 * H * W and abs(dg[0][240, 325] - 0.5) < 1e-6


def test_mesh_and_job_errors_are_errors_not_faults(ctx, lmesh):
    """A negative vertex index, a mesh without vertices, a negative mesh index and a null depth image are refused with
    P2PError before anything runs on the device; the context keeps working."""
    import ctypes as C
    from pix2pose_amd import _lib
    from pix2pose_amd.runtime import Mesh, _depth_jobs, render_depth_batch
    v, t, m = lmesh
    with pytest.raises(_lib.P2PError):
        Mesh(ctx, np.zeros((3, 3)), [[0, -1, 2]])
    with pytest.raises(_lib.P2PError):
        Mesh(ctx, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    with pytest.raises(_lib.P2PError):
        render_depth_batch(ctx, [m], [_job(np.eye(3), [0, 0, 500], mesh=-1)], H, W)
    mask = np.ones((H, W), np.uint8)
    keep = []
    arr = _depth_jobs([_job(np.eye(3), [0, 0, 500], image=0, mask=mask)], keep)
    mh = (C.c_void_p * 1)(m.handle.value)
    dp = (C.c_void_p * 1)(None)
    res = (_lib.DepthScore * 1)()
    with pytest.raises(_lib.P2PError):
        _lib.check(_lib.lib().p2p_depth_score_batch(ctx.handle, mh, 1, dp, 1, arr, 1, H, W, res, None), "p2p_depth_score_batch")
    d = render_depth_batch(ctx, [m], [_job(np.eye(3), [0, 0, 500])], H, W)[0]
    dr, margin = D.render_depth(v, t, D.K_640, np.eye(3), [0, 0, 500], H, W, with_margin=True)
    _compare(d, dr, margin)
