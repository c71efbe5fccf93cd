"""CPU tests of the depth path: the PLY reader and self-checks of the float64 restatement (tests/depth_ref.py) that the GPU
tests hold the rasteriser and the depth score to."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref as D  # noqa: E402

from pix2pose_amd.mesh import read_ply  # noqa: E402

# a unit cube's top as one quad plus a triangle, with normals / colours and an extra element the reader must skip
VERTS = np.array([[0, 0, 0], [10, 0, 0], [10, 10, 0], [0, 10, 0], [5, 5, 7.25]], np.float64)
FACES = [[0, 1, 2, 3], [0, 1, 4]]
FAN = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4]])


def _write_ascii(fn):
    lines = ["ply", "format ascii 1.0", "comment made by the test", "element vertex %d" % len(VERTS), "property float x",
             "property float y", "property float z", "property float nx", "property uchar red",
             "element face %d" % len(FACES), "property list uchar int vertex_indices", "property uchar flags",
             "element edge 1", "property int vertex1", "property int vertex2", "end_header"]
    lines += ["%g %g %g 0.5 200" % tuple(v) for v in VERTS]
    lines += ["%d %s 3" % (len(f), " ".join(map(str, f))) for f in FACES]
    lines += ["0 1"]
    open(fn, "w").write("\n".join(lines) + "\n")


def _write_binary(fn, quads_only=False):
    faces = [[0, 1, 2, 3], [1, 2, 3, 4]] if quads_only else FACES
    hdr = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(VERTS), "property float x", "property float y",
           "property float z", "property double nx", "property uchar red", "element face %d" % len(faces),
           "property list uchar int vertex_indices", "end_header"]
    b = ("\n".join(hdr) + "\n").encode()
    for v in VERTS:
        b += struct.pack("<fffdB", v[0], v[1], v[2], 0.25, 7)
    for f in faces:
        b += struct.pack("<B%di" % len(f), len(f), *f)
    open(fn, "wb").write(b)
    return faces


def test_ply_ascii_with_quads_and_extra_properties(tmp_path):
    fn = str(tmp_path / "obj_000001.ply")
    _write_ascii(fn)
    v, t = read_ply(fn)
    assert np.array_equal(v, VERTS.astype(np.float32).astype(np.float64))
    assert np.array_equal(t, FAN) and t.dtype == np.int32


def test_ply_binary_little_endian_mixed_and_quads(tmp_path):
    fn = str(tmp_path / "obj_000002.ply")
    _write_binary(fn)
    v, t = read_ply(fn)
    assert np.array_equal(v, VERTS.astype(np.float32).astype(np.float64))
    assert np.array_equal(t, FAN)
    fn2 = str(tmp_path / "obj_000003.ply")
    _write_binary(fn2, quads_only=True)         # every polygon the same size: the vectorised path
    _, t2 = read_ply(fn2)
    assert np.array_equal(t2, [[0, 1, 2], [0, 2, 3], [1, 2, 3], [1, 3, 4]])


def test_restatement_culls_back_faces_of_an_outward_mesh():
    """A closed box wound outward, 500 mm in front of the camera: the centre pixel sees the near face.  With the winding
    flipped the near face is culled and the inside of the far face is what is drawn."""
    v, t = D.box_mesh([-50, -50, -50], [50, 50, 50], 2)
    K = D.K_640
    d = D.render_depth(v, t, K, np.eye(3), [0, 0, 500], 480, 640)        # t in mm, as p2p_refine_job carries it
    j, i = int(K[1, 2]), int(K[0, 2])
    assert abs(d[j, i] - 0.45) < 1e-6
    dflip = D.render_depth(v, t[:, ::-1], K, np.eye(3), [0, 0, 500], 480, 640)
    assert abs(dflip[j, i] - 0.55) < 1e-6
    assert np.array_equal(d > 0, dflip > 0)      # same silhouette


def test_restatement_depth_of_a_tilted_plane_is_the_ray_intersection():
    """Perspective-correct depth: every covered pixel of a tilted square sits on the plane, and the shared diagonal leaves no hole."""
    verts = np.array([[-60, -60, 0], [60, -60, 0], [60, 60, 0], [-60, 60, 0]], np.float64)
    tris = np.array([[0, 1, 2], [0, 2, 3]])
    R = D.rot(0, 35) @ D.rot(1, -20)
    if (R @ [0, 0, 1])[2] > 0:                   # show the front (+z normal must face the camera)
        tris = tris[:, ::-1]
    t = np.array([0.01, -0.02, 0.4])
    K = D.K_640
    d = D.render_depth(verts, tris, K, R, t * 1000.0, 480, 640)
    n = R @ [0, 0, 1.0]
    vm = D.mesh_metres(verts).astype(np.float64)
    c = vm[0] @ R.T + t
    jj, ii = np.nonzero(d > 0)
    assert len(jj) > 5000
    rays = np.linalg.solve(K, np.stack([ii + 0.5, jj + 0.5, np.ones(len(ii))]))      # OpenGL pixel centres
    z = (c @ n) / (n @ rays)
    assert np.abs(d[jj, ii] - z).max() < 1e-6 * z.max()
    # no hole inside the projected square: pixels whose centre is well inside the quad are all covered
    P = (K @ (vm @ R.T + t).T)
    uv = (P[:2] / P[2]).T
    pu, pv = np.meshgrid(np.arange(640) + 0.5, np.arange(480) + 0.5)
    es = []
    for a in range(4):
        b = (a + 1) % 4
        du, dv = uv[b] - uv[a]
        es.append((du * (pv - uv[a, 1]) - dv * (pu - uv[a, 0])) / np.hypot(du, dv))
    es = np.array(es)
    inside = np.all(es > 1e-3, 0) | np.all(es < -1e-3, 0)
    assert inside.sum() > 5000 and np.all(d[inside] > 0)


def test_restatement_clips_and_rejects_without_failing():
    v, t = D.l_mesh(4)
    K = D.K_640
    # straddling the near plane and far out of the image: nothing raises, depths stay within the clip range
    for tt in ([0, 0, 20], [3000, 0, 300], [0, 0, 12000], [0, 0, -1000]):
        d = D.render_depth(v, t, K, D.rot(1, 10), tt, 480, 640)
        assert np.all((d == 0) | ((d >= 0.01) & (d <= 10)))
    assert not D.render_depth(v, t, K, np.eye(3), [0, 0, 12000], 480, 640).any()        # beyond the far plane
    assert not D.render_depth(v, t, K, np.eye(3), [0, 0, -1000], 480, 640).any()        # behind the camera


def test_unit_quirk_of_render_obj_is_kept():
    """render_obj gets tra_pred/1000 and divides once more when that exceeds 100 (icp3d.py:46): a t_z beyond 100 m is drawn 1000x nearer."""
    v, t = D.l_mesh(2)
    a = D.render_depth(v, t, D.K_640, D.rot(2, 30), [10000.0, -5000.0, 700000.0], 480, 640)
    b = D.render_depth(v, t, D.K_640, D.rot(2, 30), [10.0, -5.0, 700.0], 480, 640)
    both = (a > 0) & (b > 0)
    assert both.sum() > 100 and ((a > 0) != (b > 0)).sum() <= 5          # the two divisions round differently: edge centres may flip
    assert np.abs(a[both] - b[both]).max() <= 1e-6 * b.max()


def test_tie_rule_gives_every_centre_exactly_one_write():
    """Vertices exactly on pixel centres: all edges run through centres.  Counted independently of the depth: every centre of
    the 64 x 64 px square is written by exactly one triangle (no hole on a shared edge, no double write), and of each pair of
    opposite outer edges exactly one owns its centres, so the square covers exactly 64 x 64 pixels."""
    v, t = D.pixel_grid_mesh()
    vm = D.mesh_metres(v)
    assert set(np.unique(vm[:, :2])) == {-0.5, -0.25, 0.0, 0.25, 0.5}            # exact: the vertices sit on centres
    d, counts = D.render_depth(v, t, D.GRID_K, np.eye(3), [0, 0, 1000], 480, 640, with_counts=True)
    assert counts.max() == 1 and counts.sum() == 64 * 64
    jj, ii = np.nonzero(counts)
    assert ii.max() - ii.min() == 63 and jj.max() - jj.min() == 63
    assert np.all(d[counts == 1] == 1.0) and not d[counts == 0].any()


def test_depth_score_restatement_by_hand():
    ref = np.array([[0.5, 0.5, 0.0], [0.5, 0.6, 0.7]], np.float32)
    tgt = np.array([[0.51, 0.5, 0.3], [0.525, 0.6, 0.0]], np.float32)
    m = np.array([[1, 1, 1], [1, 0, 1]], np.uint8)
    s, inl = D.depth_score(ref, tgt, m)
    assert s["union"] == 5 and s["inlier_count"] == 2
    assert np.array_equal(inl, [[True, True, False], [False, False, False]])
    d = np.abs(np.float64(np.float32(0.51)) - np.float64(np.float32(0.5)))
    assert abs(s["fcn"] - ((0.02 - d) / 0.02 + 1.0)) < 1e-12
    assert s["ratio"] == 2 / 5


# --- the restatement against oracles that do not share its derivation (depth_ref: gl_window, raycast_depth, score_ref32) ---

def test_gl_transform_gives_the_restatements_pixel_coordinates():
    """The reference's matrices (build_projection, yz_flip, viewport, row flip) put every vertex where the restatement's
    u = fx x/z + s y/z + cx, v = fy y/z + cy does, with skew of both signs, fx != fy, off-centre principal points and four sizes."""
    v, _ = D.l_mesh(2)
    rs = np.random.RandomState(11)
    worst = 0.0
    for K, H, W in D.CAMERAS:
        for _ in range(20):
            R, t = D.random_pose(rs, K, H, W)
            u, vv, _ = D.project(v, K, R, t)
            gu, gv, _ = D.gl_window(v, K, R, t, H, W)
            worst = max(worst, np.abs(gu - u).max(), np.abs(gv - vv).max())
    assert worst <= 1e-9, worst


def test_gl_front_faces_are_the_restatements_negative_area_faces():
    """GL draws triangles counter-clockwise in the window (y_w up); the restatement draws negative (u, v) area (v down)."""
    v, t = D.l_mesh(2)
    rs = np.random.RandomState(12)
    n_front = n_all = 0
    for K, H, W in D.CAMERAS:
        for _ in range(20):
            R, tt = D.random_pose(rs, K, H, W)
            u, vv, z = D.project(v, K, R, tt)
            gu, gv, _ = D.gl_window(v, K, R, tt, H, W)
            xw, yw = gu, H - gv
            ok = np.all(z[t] >= D.CLIP_NEAR, axis=1)
            a_img = (u[t[:, 1]] - u[t[:, 0]]) * (vv[t[:, 2]] - vv[t[:, 0]]) - (u[t[:, 2]] - u[t[:, 0]]) * (vv[t[:, 1]] - vv[t[:, 0]])
            a_gl = (xw[t[:, 1]] - xw[t[:, 0]]) * (yw[t[:, 2]] - yw[t[:, 0]]) - (xw[t[:, 2]] - xw[t[:, 0]]) * (yw[t[:, 1]] - yw[t[:, 0]])
            clear = ok & (np.abs(a_img) > 1e-6)          # edge-on faces are a rounding question, not an orientation rule
            assert np.array_equal((a_gl > 0)[clear], (a_img < 0)[clear])
            n_front += int((a_img < 0)[clear].sum())
            n_all += int(clear.sum())
    assert 0.3 * n_all < n_front < 0.7 * n_all


def test_gl_depth_readback_returns_the_eye_depth():
    """finish()'s mult / (d_w + addi) in float32 on the exact window depth gives the eye depth the restatement interpolates.
    Measured: at most 6.7e-6 relative over 0.2-2.2 m (float32 rounding of d_w near 1, amplified by the cancellation in d_w + addi)."""
    z = np.linspace(200.0, 2200.0, 100001)
    rs = np.random.RandomState(13)
    worst = 0.0
    for K, H, W in D.CAMERAS:
        verts = np.stack([rs.uniform(-0.3, 0.3, z.size) * z, rs.uniform(-0.3, 0.3, z.size) * z, z], 1)
        _, _, zc = D.project(verts, K, np.eye(3), [0, 0, 0])
        _, _, d_w = D.gl_window(verts, K, np.eye(3), [0, 0, 0], H, W)
        assert np.all((d_w > 0) & (d_w < 1))
        worst = max(worst, float(np.abs(D.gl_readback_depth(d_w) / zc - 1).max()))
    assert worst <= 1e-5, worst


def _raycast_window(dr, K, verts, R, t, H, W, pad=3):
    """The pixel box of the projected vertices (all in front of the camera), padded: the triangles' images lie inside it."""
    u, v, z = D.project(verts, K, R, t)
    assert np.all(z > D.CLIP_NEAR)
    return (max(0, int(np.floor(v.min())) - pad), min(H, int(np.ceil(v.max())) + pad),
            max(0, int(np.floor(u.min())) - pad), min(W, int(np.ceil(u.max())) + pad))


def test_raycast_oracle_matches_the_restatement():
    """A ray caster in camera space (no projection of edges, no edge functions) draws what render_depth draws: depth to float32
    rounding, coverage everywhere but at centres within either renderer's edge margin."""
    rs = np.random.RandomState(14)
    meshes = [D.l_mesh(2), D.box_mesh([-50, -30, -20], [50, 30, 20], 2), D.box_mesh([-25, -25, -25], [25, 25, 25], 1)]
    n_cov = worst = 0
    for K, H, W in D.CAMERAS:
        for k in range(6):
            verts, tris = meshes[k % len(meshes)]
            R, t = D.random_pose(rs, K, H, W, 0.3, 0.9)
            dr, m1 = D.render_depth(verts, tris, K, R, t, H, W, with_margin=True)
            win = _raycast_window(dr, K, verts, R, t, H, W)
            rc, m2 = D.raycast_depth(verts, tris, K, R, t, H, W, window=win)
            sub, msub = dr[win[0]:win[1], win[2]:win[3]], m1[win[0]:win[1], win[2]:win[3]]
            assert (dr > 0).sum() == (sub > 0).sum()            # nothing drawn outside the vertices' box
            away = ~(msub | m2)
            assert np.array_equal((sub > 0) & away, (rc > 0) & away)
            both = (sub > 0) & (rc > 0) & away
            rel = np.abs(sub[both] - rc[both]) / rc[both]
            assert rel.max(initial=0) <= 2.0 ** -23, rel.max()
            n_cov += int(both.sum())
            worst = max(worst, rel.max(initial=0))
    print("ray cast vs restatement: %d centres, depth within %.1e relative" % (n_cov, worst))
    assert n_cov > 20000


def test_raycast_oracle_sees_the_clip_rules():
    """Whole-triangle near rejection and the far clip, as the ray caster states them, agree with the restatement."""
    v, t = D.l_mesh(2)
    K, H, W = D.CAMERAS[3]
    for R, tt in ((D.rot(1, 15), [0, 0, 25]), (np.eye(3), [0, 0, 9990]), (np.eye(3), [0, 0, 10020]), (np.eye(3), [0, 0, -500])):
        dr, m1 = D.render_depth(v, t, K, R, tt, H, W, with_margin=True)
        rc, m2 = D.raycast_depth(v, t, K, R, tt, H, W)
        away = ~(m1 | m2)
        assert np.array_equal((dr > 0) & away, (rc > 0) & away)
    assert not rc.any()                          # the last pose: behind the camera


def _threshold_pairs(rs, n):
    """Rendered / sensor float32 pairs in 0.2-2.2 m with dt the float32 nearest dr + 0.02, or one ulp below or above it, so
    |dr - dt| lands on both sides of the inlier threshold."""
    dr = rs.uniform(0.2, 2.15, n).astype(np.float32)
    dt = (dr + np.float32(0.02)).astype(np.float32)
    step = rs.randint(-1, 2, n)
    dt = np.where(step < 0, np.nextafter(dt, np.float32(0)), np.where(step > 0, np.nextafter(dt, np.float32(np.inf)), dt))
    return dr, dt.astype(np.float32)


def test_float32_reference_score_counts_equal_the_float64_score():
    """The reference scores float32 maps in float32; the kernel and the restatement in float64.  Counts and masks agree: for depths
    in 0.2-2.2 m with |dr - dt| near 0.02 the float32 difference is exact (Sterbenz: the operands are within a factor 2), a
    multiple of 2^-26, and float32(0.02) is not one, so '< 0.02' in float64 and '< float32(0.02)' see the same value on the same
    side.  fcn differs only by float32 rounding (float32(0.02) != 0.02 in every term) and pairwise summation: measured 1.4e-8 per
    union pixel here, asserted <= 1e-7 per union pixel."""
    rs = np.random.RandomState(15)
    H, W = 37, 53
    worst = 0.0
    for trial in range(20):
        dr, dt = _threshold_pairs(rs, H * W)
        swap = rs.rand(H * W) < 0.5
        dr, dt = np.where(swap, dt, dr).reshape(H, W), np.where(swap, dr, dt).reshape(H, W)
        if trial % 2:
            dt = dt + rs.normal(0, 0.01, dt.shape).astype(np.float32)
            dt = np.clip(dt, 0.2, 2.2).astype(np.float32)
        mask = rs.rand(H, W) < 0.8
        s64, m64 = D.depth_score(dr, dt, mask)
        s32, m32 = D.score_ref32(dr, dt, mask)
        assert s64["inlier_count"] == s32["inlier_count"] and s64["union"] == s32["union"]
        assert np.array_equal(m64, m32)
        assert 0 < s64["inlier_count"] < s64["union"]
        worst = max(worst, abs(float(s32["fcn"]) - s64["fcn"]) / s64["union"])
    print("fcn float32 - float64: %.2e per union pixel" % worst)
    assert worst <= 1e-7, worst


def test_threshold_ulps_fall_on_both_sides():
    """The constructed pairs above do straddle the threshold: one ulp below is an inlier, one ulp above is not."""
    dr = np.float32(0.75)
    lo = np.float32(dr + np.float32(0.02))
    while abs(np.float64(lo) - np.float64(dr)) >= 0.02:
        lo = np.nextafter(lo, np.float32(0))
    hi = np.nextafter(lo, np.float32(np.inf))
    assert np.float32(lo) - dr < 0.02 <= np.float64(hi) - np.float64(dr)
    s, _ = D.depth_score(np.array([[dr, dr]], np.float32), np.array([[lo, hi]], np.float32), np.ones((1, 2), bool))
    s32, _ = D.score_ref32(np.array([[dr, dr]], np.float32), np.array([[lo, hi]], np.float32), np.ones((1, 2), bool))
    assert s["inlier_count"] == s32["inlier_count"] == 1


def test_nan_sensor_pixel_rule():
    """The NaN rule (depth_ref docstring): counted in the union, not an inlier, adds 0 to fcn."""
    dr = np.array([[0.5, 0.5, 0.5]], np.float32)
    dt = np.array([[0.5, np.nan, 0.51]], np.float32)
    s, inl = D.depth_score(dr, dt, np.ones((1, 3), bool))
    assert s["union"] == 3 and s["inlier_count"] == 2 and not inl[0, 1]
    d = np.float64(np.float32(0.51)) - 0.5
    assert abs(s["fcn"] - (1.0 + (0.02 - d) / 0.02)) < 1e-12
