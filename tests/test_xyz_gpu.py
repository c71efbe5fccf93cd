"""GPU tests of the XYZ colour rasteriser (csrc/depth.hip: p2p_mesh_set_colors, p2p_render_xyz_batch):
its depth against p2p_render_depth_batch bit for bit, its colour against the float64 restatement (tests/xyz_ref.py), the winner
rule and its independence of order, batch and route, the device-side bounding box, and the argument checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref as D  # noqa: E402
import xyz_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu

COLOR_TOL = 2.0 ** -22      # colours are in [0, 1], computed in fp64 and stored as float32 (half an ulp below 1 is 2^-25)


@pytest.fixture(scope="module")
def ctx():
    from pix2pose_amd.runtime import Context
    c = Context(0, max_batch=8)
    yield c
    c.close()


def _xyz_mesh(ctx, v, t, flat=False):
    from pix2pose_amd.runtime import Mesh
    from pix2pose_amd.xyz_model import xyz_colors
    # (a flat mesh has no coordinate to encode along its normal: random colours)
    c = np.random.RandomState(len(v)).randint(0, 256, (len(v), 3)).astype(np.uint8) if flat else xyz_colors(v)[0]
    m = Mesh(ctx, v, t)
    m.set_colors(c)
    return v, t, c, m


@pytest.fixture(scope="module")
def meshes(ctx):
    """Meshes of different sizes with their XYZ colours: the L shape (1536 triangles), a coarse box (108), a fine box (3072)."""
    return [_xyz_mesh(ctx, *D.l_mesh(8)), _xyz_mesh(ctx, *D.box_mesh([-40, -30, -15], [40, 30, 15], 3)),
            _xyz_mesh(ctx, *D.box_mesh([-25, -60, -20], [25, 60, 20], 16))]


def _job(R, t, K, mesh=0):
    return {"mesh": mesh, "camK": K, "R": R, "t": t}


def _jobs(n, K, H, W, seed, n_meshes, zlo=0.35, zhi=1.2):
    rs = np.random.RandomState(seed)
    return [_job(*D.random_pose(rs, K, H, W, zlo, zhi), K, mesh=k % n_meshes) for k in range(n)]


def _plane(n, side_mm):
    g = np.linspace(-side_mm / 2, side_mm / 2, n + 1)
    verts = np.array([(x, y, 0.0) for y in g for x in g])
    tris = []
    for a in range(n):
        for b in range(n):
            q = [a * (n + 1) + b, a * (n + 1) + b + 1, (a + 1) * (n + 1) + b + 1, (a + 1) * (n + 1) + b]
            tris += [(q[0], q[2], q[1]), (q[0], q[3], q[2])]
    return verts, np.array(tris)


# ---- depth identity --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", [0, 3])
def test_depth_is_bit_identical_to_the_depth_path(ctx, meshes, cam):
    """Skew of both signs, fx != fy, off-centre principal points; 640 x 480 and 53 x 37."""
    from pix2pose_amd.runtime import render_depth_batch, render_xyz_batch
    K, H, W = D.CAMERAS[cam]
    z = (0.35, 1.2) if cam == 0 else (0.08, 0.3)
    jobs = _jobs(12, K, H, W, 20 + cam, len(meshes), *z)
    jobs.append(_job(D.rot(0, 30), [0.0, 0.0, 45.0], K))              # 10 mm in front of the camera: big-box triangles
    jobs.append(_job(D.rot(2, 5), [3000.0, 0.0, 300.0], K))           # outside the image: empty
    ms = [m[3] for m in meshes]
    color, depth, bbox = render_xyz_batch(ctx, ms, jobs, H, W)
    want = render_depth_batch(ctx, ms, jobs, H, W)
    assert np.array_equal(depth.view(np.uint32), want.view(np.uint32))
    assert (depth[:12] > 0).sum() > 12 * 20 and not depth[-1].any()
    assert np.all(color[depth == 0] == 0) and color.min() >= 0 and color.max() <= 1


def test_depth_identity_in_a_batch_of_256_jobs(ctx, meshes):
    from pix2pose_amd.runtime import render_depth_batch, render_xyz_batch
    K, H, W = D.CAMERAS[0]
    jobs = _jobs(256, K, H, W, 31, len(meshes))
    ms = [m[3] for m in meshes]
    color, depth, bbox = render_xyz_batch(ctx, ms, jobs, H, W)
    want = render_depth_batch(ctx, ms, jobs, H, W)
    assert np.array_equal(depth.view(np.uint32), want.view(np.uint32))
    assert (depth > 0).sum(axis=(1, 2)).min() > 100
    for k in range(0, 256, 17):                                        # the box of every 17th job (all of them: the bbox test)
        assert bbox[k].tolist() == X.bbox_of(depth[k]).tolist()
    # a job of the batch alone: same bits
    for k in (0, 100, 255):
        c1, d1, b1 = render_xyz_batch(ctx, ms, [jobs[k]], H, W)
        assert np.array_equal(c1[0].view(np.uint32), color[k].view(np.uint32)) and np.array_equal(d1[0], depth[k])
        assert np.array_equal(b1[0], bbox[k])


def test_depth_identity_with_more_than_1024_big_box_triangles(ctx):
    """The 20 x 20-quad plane of test_depth_gpu.py close to the camera: every triangle's box holds more than 1024 centres, so
    the big-box route gets more list entries than it has workgroups."""
    from pix2pose_amd.runtime import render_depth_batch, render_xyz_batch
    h, w = 960, 1280
    K = np.array([[500.0, 0.0, 640.0], [0.0, 500.0, 480.0], [0.0, 0.0, 1.0]])
    v, t, c, m = _xyz_mesh(ctx, *_plane(20, 800.0), flat=True)
    jobs = [_job(np.eye(3), [0, 0, 500], K), _job(D.rot(0, 20) @ D.rot(1, -15), [20, -30, 520], K),
            _job(D.rot(2, 40), [-50, 10, 480], K)]
    color, depth, bbox = render_xyz_batch(ctx, [m], jobs, h, w)
    want = render_depth_batch(ctx, [m], jobs, h, w)
    assert np.array_equal(depth.view(np.uint32), want.view(np.uint32))
    assert all((depth[k] > 0).sum() > 0.3 * h * w for k in range(3))
    cr, dr, owner, margin = X.render_xyz(v, t, c, K, jobs[1]["R"], jobs[1]["t"], h, w)
    _compare_color(color[1], depth[1], cr, dr, margin)


# ---- colour parity ---------------------------------------------------------------------------------------------------------

def _compare_color(cg, dg, cr, dr, margin):
    """Away from edges both renders have the same owner by rule: the colours agree to COLOR_TOL.  A centre within 1e-4 px of an
    edge may be owned by another triangle (or by none) on the device: such centres are counted and capped by the number of margin
    centres -- the allowance of test_depth_gpu.py (_compare: coverage may differ inside the margin only)."""
    both = (dg > 0) & (dr > 0)
    diff = np.abs(cg.astype(np.float64) - cr.astype(np.float64)).max(axis=2)
    bad = (both & (diff > COLOR_TOL)) | ((dg > 0) != (dr > 0))
    assert not np.any(bad & ~margin), ("colour differs away from an edge", np.argwhere(bad & ~margin)[:5], diff[bad & ~margin][:5])
    assert int(bad.sum()) <= int(margin.sum())
    return int(bad.sum()), float(diff[both & ~margin].max(initial=0))


@pytest.mark.parametrize("cam", [0, 3])
def test_colour_equals_the_restatement(ctx, meshes, cam):
    from pix2pose_amd.runtime import render_xyz_batch
    K, H, W = D.CAMERAS[cam]
    z = (0.35, 0.9) if cam == 0 else (0.08, 0.3)
    jobs = _jobs(6, K, H, W, 40 + cam, len(meshes), *z)
    jobs.append(_job(D.rot(0, 40), [250.0, 100.0, 400.0] if cam == 0 else [30.0, 10.0, 120.0], K))      # partly outside the image
    color, depth, bbox = render_xyz_batch(ctx, [m[3] for m in meshes], jobs, H, W)
    n_edge, worst, n_px = 0, 0.0, 0
    for k, j in enumerate(jobs):
        v, t, c, _ = meshes[j["mesh"]]
        cr, dr, owner, margin = X.render_xyz(v, t, c, K, j["R"], j["t"], H, W)
        e, w = _compare_color(color[k], depth[k], cr, dr, margin)
        n_edge += e
        worst = max(worst, w)
        n_px += int((dr > 0).sum())
    print("covered %d px, edge-grazing differences %d, worst colour difference %.3e" % (n_px, n_edge, worst))
    assert n_px > (20000 if cam == 0 else 500)


# ---- the winner rule and order independence -------------------------------------------------------------------------------

def _pair_scene(perm_seed=None, swap=False):
    """Two coplanar overlapping triangles of different colours (indices 0 and 1) in front of a box; the box's triangles optionally
    permuted.  Seen through depth_ref.GRID_K at t = (0, 0, 1000) mm."""
    pv = np.array([[-250, -250, 0], [250, -250, 0], [0, 250, 0], [-250, 250, 0], [250, 250, 0], [0, -250, 0]], np.float64)
    pt = np.array([[0, 2, 1], [3, 4, 5]])
    pc = np.array([[255, 0, 0]] * 3 + [[0, 0, 255]] * 3, np.uint8)
    if swap:
        pt = pt[::-1]
    bv, bt = D.box_mesh([-400, -300, 100], [400, 300, 300], 4)
    if perm_seed is not None:
        bt = bt[np.random.RandomState(perm_seed).permutation(len(bt))]
    bc = np.random.RandomState(9).randint(0, 256, (len(bv), 3)).astype(np.uint8)
    return np.concatenate([pv, bv]), np.concatenate([pt, bt + len(pv)]), np.concatenate([pc, bc])


def test_equal_depth_shows_the_lower_index_and_order_does_not_matter(ctx):
    from pix2pose_amd.runtime import Mesh, render_xyz_batch
    K, H, W = D.GRID_K, 480, 640
    pose = (np.eye(3), [0.0, 0.0, 1000.0])
    tilt = (D.rot(0, 12) @ D.rot(1, -9), [20.0, -10.0, 1100.0])
    outs = []
    for seed in (None, 1, 2):
        v, t, c = _pair_scene(seed)
        m = Mesh(ctx, v, t)
        m.set_colors(c)
        jobs = [_job(*pose, K), _job(*tilt, K)]
        color, depth, bbox = render_xyz_batch(ctx, [m], jobs, H, W)
        outs.append((color, depth, bbox))
        if seed is None:
            cr, dr, owner, margin = X.render_xyz(v, t, c, K, *pose, H, W)
            a = D.render_depth(v, t[0:1], K, *pose, H, W) > 0
            b = D.render_depth(v, t[1:2], K, *pose, H, W) > 0
            both = a & b
            assert both.sum() > 100
            assert np.all(depth[0][both] == np.float32(1.0))                        # the same float32 depth from both triangles
            assert np.all(color[0][both] == np.float32([1, 0, 0]))                  # triangle 0 (red) owns the overlap
            assert np.all(color[0][b & ~a] == np.float32([0, 0, 1]))
            _compare_color(color[0], depth[0], cr, dr, margin)
            # repeating the call, a job alone, the batch split
            again = render_xyz_batch(ctx, [m], jobs, H, W)
            for x, y in zip(again, outs[0]):
                assert np.array_equal(x, y)
            for k in range(2):
                alone = render_xyz_batch(ctx, [m], [jobs[k]], H, W)
                assert np.array_equal(alone[0][0].view(np.uint32), color[k].view(np.uint32))
                assert np.array_equal(alone[1][0], depth[k]) and np.array_equal(alone[2][0], bbox[k])
    for color, depth, bbox in outs[1:]:                                            # the other triangles permuted: same bits
        assert np.array_equal(color.view(np.uint32), outs[0][0].view(np.uint32))
        assert np.array_equal(depth, outs[0][1]) and np.array_equal(bbox, outs[0][2])
    # the pair swapped: now the blue triangle has index 0
    v, t, c = _pair_scene(None, swap=True)
    m = Mesh(ctx, v, t)
    m.set_colors(c)
    color, depth, _ = render_xyz_batch(ctx, [m], [_job(*pose, K)], H, W)
    assert np.all(color[0][both] == np.float32([0, 0, 1])) and np.array_equal(depth[0], outs[0][1][0])


def test_tie_between_the_routes_is_decided_by_index(ctx):
    """The overlap once more with triangle 0 cut into many small triangles (the small-box route) under one large triangle of a
    higher index (the big-box route), and the other way round: the lower index owns every shared centre either way."""
    from pix2pose_amd.runtime import Mesh, render_xyz_batch
    K, H, W = D.GRID_K, 480, 640
    gv, gt = _plane(32, 800.0)                     # 25 mm quads, 1.6 px wide: the small-box route; facing -z like the big one
    big_v = np.array([[-500, -500, 0], [500, -500, 0], [0, 500, 0]], np.float64)      # covers > 1024 centres: the big-box route
    big_t = np.array([[0, 2, 1]])
    for big_first in (False, True):
        if big_first:
            v, t = np.concatenate([big_v, gv]), np.concatenate([big_t, gt + 3])
            c = np.concatenate([np.uint8([[0, 255, 0]] * 3), np.uint8([[255, 0, 255]] * len(gv))])
        else:
            v, t = np.concatenate([gv, big_v]), np.concatenate([gt, big_t + len(gv)])
            c = np.concatenate([np.uint8([[255, 0, 255]] * len(gv)), np.uint8([[0, 255, 0]] * 3)])
        m = Mesh(ctx, v, t)
        m.set_colors(c)
        color, depth, _ = render_xyz_batch(ctx, [m], [_job(np.eye(3), [0.0, 0.0, 1000.0], K)], H, W)
        cr, dr, owner, margin = X.render_xyz(v, t, c, K, np.eye(3), [0.0, 0.0, 1000.0], H, W)
        a = D.render_depth(big_v, big_t, K, np.eye(3), [0.0, 0.0, 1000.0], H, W) > 0
        b = D.render_depth(gv, gt, K, np.eye(3), [0.0, 0.0, 1000.0], H, W) > 0
        both = a & b
        assert both.sum() > 1024 and a.sum() > 1024
        assert np.all(color[0][both] == np.float32([0, 1, 0] if big_first else [1, 0, 1]))
        assert np.array_equal(color[0], cr) and np.array_equal(depth[0], dr)       # exact geometry: no edge allowance


# ---- bounding box ----------------------------------------------------------------------------------------------------------

def test_bbox_equals_numpy_on_the_returned_depth(ctx, meshes):
    from pix2pose_amd.runtime import render_xyz_batch
    K, H, W = D.CAMERAS[0]
    jobs = _jobs(10, K, H, W, 50, len(meshes))
    jobs += [_job(D.rot(2, 5), [3000.0, 0.0, 300.0], K),               # outside the image: empty
             _job(np.eye(3), [0.0, 0.0, -500.0], K),                   # behind the camera: empty
             _job(D.rot(0, 40), [250.0, 100.0, 400.0], K),             # cut by the image border
             _job(D.rot(0, 30), [0.0, 0.0, 45.0], K)]                  # fills the image
    color, depth, bbox = render_xyz_batch(ctx, [m[3] for m in meshes], jobs, H, W)
    assert bbox.dtype == np.int32 and bbox.shape == (len(jobs), 4)
    for k in range(len(jobs)):
        assert bbox[k].tolist() == X.bbox_of(depth[k]).tolist(), k
    assert bbox[10].tolist() == [-1, -1, -1, -1] and bbox[11].tolist() == [-1, -1, -1, -1]
    assert bbox[12][3] == W - 1 or bbox[12][2] == H - 1
    for cam in (3,):
        K, H, W = D.CAMERAS[cam]
        jobs = _jobs(5, K, H, W, 51, len(meshes), 0.08, 0.3)
        color, depth, bbox = render_xyz_batch(ctx, [m[3] for m in meshes], jobs, H, W)
        for k in range(len(jobs)):
            assert bbox[k].tolist() == X.bbox_of(depth[k]).tolist(), k


# ---- argument errors -------------------------------------------------------------------------------------------------------

def test_argument_errors_are_errors_not_faults(ctx, meshes):
    import ctypes as C
    from pix2pose_amd import _lib
    from pix2pose_amd.runtime import Mesh, _depth_jobs, render_xyz_batch
    K, H, W = D.CAMERAS[3]
    v, t, c, m = meshes[1]
    L = _lib.lib()
    job = _job(np.eye(3), [0.0, 0.0, 150.0], K)
    plain = Mesh(ctx, v, t)                                            # no colours
    arr = _depth_jobs([job], [])
    color = np.zeros((1, H, W, 3), np.float32)
    mh = (C.c_void_p * 1)(plain.handle.value)
    rc = L.p2p_render_xyz_batch(ctx.handle, mh, 1, arr, 1, H, W, color.ctypes.data, None, None)
    assert rc == -1 and b"no colours" in L.p2p_last_error()            # P2P_ERR_INVALID_ARG
    with pytest.raises(_lib.P2PError, match="no colours"):
        render_xyz_batch(ctx, [plain], [job], H, W)
    rc = L.p2p_mesh_set_colors(plain.handle, c.ctypes.data, len(c) - 1)
    assert rc == -1 and b"vertices" in L.p2p_last_error()
    with pytest.raises(_lib.P2PError):
        plain.set_colors(c[:-1])
    assert L.p2p_mesh_set_colors(plain.handle, None, len(c)) == -1 and L.p2p_last_error()
    with pytest.raises(ValueError):
        plain.set_colors(c.astype(np.float32))
    mh = (C.c_void_p * 1)(m.handle.value)
    rc = L.p2p_render_xyz_batch(ctx.handle, mh, 1, arr, 1, H, W, None, None, None)
    assert rc == -1 and b"colour buffer" in L.p2p_last_error()
    assert L.p2p_render_xyz_batch(ctx.handle, mh, 1, arr, 1, 0, W, color.ctypes.data, None, None) == -1
    assert L.p2p_render_xyz_batch(None, mh, 1, arr, 1, H, W, color.ctypes.data, None, None) == -1
    # depth and bbox may be null; the context keeps working and the late colours take effect
    assert L.p2p_render_xyz_batch(ctx.handle, mh, 1, arr, 1, H, W, color.ctypes.data, None, None) == 0
    plain.set_colors(c)
    c2, d2, b2 = render_xyz_batch(ctx, [plain], [job], H, W)
    assert np.array_equal(c2[0], color[0]) and d2.any() and b2[0].tolist() == X.bbox_of(d2[0]).tolist()
    cr, dr, owner, margin = X.render_xyz(v, t, c, K, np.eye(3), [0.0, 0.0, 150.0], H, W)
    _compare_color(c2[0], d2[0], cr, dr, margin)


# ---- patch builder ---------------------------------------------------------------------------------------------------------

def _frames(n, H, W, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n)]


def _exp_sensitive(h, w):
    """The library builds its Gaussian weights with libm's exp, the scipy of this interpreter with numpy's SIMD exp, 1 ulp apart on
    some arguments (tests/test_est_pose_gpu.py: _exp_sensitive_sides).  True when the weights of a h x w crop's two axes differ
    between the two; such a job is held to its shape only, as that file does."""
    import math
    oh, ow = X.patch_shape(h, w)
    for n_in, n_out in ((h, oh), (w, ow)):
        sigma = (n_in / n_out - 1) / 2
        r = int(4.0 * sigma + 0.5) if sigma > 0 else 0
        if r <= 0:
            continue
        c = -0.5 / (sigma * sigma)
        x = np.arange(-r, r + 1)
        if not np.array_equal(np.exp(c * x ** 2), np.array([math.exp(c * float(k * k)) for k in x])):
            return True
    return False


@pytest.mark.parametrize("gen", [0, 1, 2])
def test_patches_equal_the_restatement(ctx, meshes, gen):
    """Every scikit-image generation of the resize (0: <= 0.14; 1: 0.17 / 0.18, filtered and warped in float32; 2: 0.15 / 0.16,
    filtered, warped in double).  Unresized patches (max side <= 128) match on the integers exactly.  Resized ones too: the criterion of the existing resize
    tests (tests/test_external_vectors.py::test_hip_back_resize_matches_real_skimage and the oracle comparisons of
    tests/test_est_pose_gpu.py) is bit for bit, with no flip allowance.  Shapes are exact; the empty render is reported and not
    written."""
    from pix2pose_amd.runtime import render_xyz_batch, xyz_patch_batch
    K, H, W = D.CAMERAS[0]
    rs = np.random.RandomState(60)
    jobs = [_job(*D.random_pose(rs, K, H, W, 0.7, 1.2), K, mesh=k % 3) for k in range(5)]        # small boxes
    jobs += [_job(*D.random_pose(rs, K, H, W, 0.2, 0.33), K, mesh=k % 3) for k in range(5)]      # boxes above 128 px
    jobs.append(_job(D.rot(2, 5), [3000.0, 0.0, 300.0], K))                                      # empty
    frames = _frames(len(jobs), H, W, 61)
    color, depth, bbox = render_xyz_batch(ctx, [m[3] for m in meshes], jobs, H, W)
    patches = xyz_patch_batch(ctx, frames, color, depth, bbox, gen)
    n_small = n_big = n_sensitive = 0
    for k in range(len(jobs)):
        want = X.patch(frames[k], color[k], depth[k], bbox[k], gen)
        if want is None:
            assert patches[k] is None
            continue
        h, w = bbox[k][2] - bbox[k][0], bbox[k][3] - bbox[k][1]
        assert patches[k].shape == want.shape == X.patch_shape(h, w) + (6,) and patches[k].dtype == np.uint8
        assert max(patches[k].shape[:2]) <= 128
        diff = patches[k].astype(int) - want.astype(int)
        print("job %d: box %d x %d -> %s, differing bytes %d (max %d)" % (k, h, w, want.shape[:2], (diff != 0).sum(), np.abs(diff).max()))
        if gen > 0 and max(h, w) > 128 and _exp_sensitive(h, w):
            n_sensitive += 1
            continue
        assert np.array_equal(patches[k], want)
        n_small += max(h, w) <= 128
        n_big += max(h, w) > 128
    print("exp-sensitive jobs held to their shape: %d" % n_sensitive)
    assert patches[-1] is None and n_small >= 3 and n_big + n_sensitive >= 3 and n_big >= 2
    # a box with a zero side is skipped as well, and a job alone gives the same bytes
    b2 = bbox.copy()
    b2[0, 2] = b2[0, 0]
    assert xyz_patch_batch(ctx, frames[:1], color[:1], depth[:1], b2[:1], gen)[0] is None
    alone = xyz_patch_batch(ctx, frames[6:7], color[6:7], depth[6:7], bbox[6:7], gen)[0]
    assert np.array_equal(alone, patches[6])


def test_patch_argument_errors(ctx, meshes):
    from pix2pose_amd import _lib
    from pix2pose_amd.runtime import render_xyz_batch, xyz_patch_batch
    K, H, W = D.CAMERAS[3]
    jobs = [_job(np.eye(3), [0.0, 0.0, 150.0], K, mesh=1)]
    frames = _frames(1, H, W, 62)
    color, depth, bbox = render_xyz_batch(ctx, [m[3] for m in meshes], jobs, H, W)
    with pytest.raises(_lib.P2PError, match="generation"):
        xyz_patch_batch(ctx, frames, color, depth, bbox, 3)
    bad = bbox.copy()
    bad[0, 3] = W
    with pytest.raises(_lib.P2PError, match="outside"):
        xyz_patch_batch(ctx, frames, color, depth, bad, 0)
    L = _lib.lib()
    assert L.p2p_xyz_patch_batch(ctx.handle, None, color.ctypes.data, depth.ctypes.data, bbox.ctypes.data, 1, H, W, 0, None, None) == -1
    assert xyz_patch_batch(ctx, frames, color, depth, bbox, 0)[0] is not None


# ---- driver ----------------------------------------------------------------------------------------------------------------

def test_make_train_xyz_on_a_synthetic_bop_tree(tmp_path):
    """Two objects (object 2 with a continuous symmetry about z), four training images: images 0, 1, 3 have object 1 first, image 2
    object 2.  Files are numbered per object as the reference's xyz_id; each equals the restatement's patch."""
    import json
    from PIL import Image
    from pix2pose_amd import make_train_xyz
    from pix2pose_amd.mesh import write_ply_rgb
    from pix2pose_amd.xyz_model import get_sympose, read_xyz_model
    K, H, W = D.K_640, 480, 640
    root = tmp_path / "bop" / "lmo"
    (root / "models").mkdir(parents=True)
    geo = {1: D.l_mesh(4), 2: D.box_mesh([-40, -30, -15], [40, 30, 15], 3)}
    for oid, (v, t) in geo.items():
        write_ply_rgb(str(root / "models" / ("obj_%06d.ply" % oid)), v, t, np.zeros((len(v), 3), np.uint8))
    info = {"1": {"diameter": 100.0}, "2": {"diameter": 100.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}
    (root / "models" / "models_info.json").write_text(json.dumps(info))
    (root / "camera.json").write_text(json.dumps({"fx": 1.0, "fy": 1.0, "cx": 0.0, "cy": 0.0, "width": W, "height": H, "depth_scale": 1.0}))
    scene = root / "train" / "000001"
    (scene / "rgb").mkdir(parents=True)
    rs = np.random.RandomState(70)
    first = [1, 1, 2, 1]
    zr = [(0.7, 1.0), (0.2, 0.3), (0.2, 0.3), (0.7, 1.0)]
    frames, gts, cams = _frames(4, H, W, 71), {}, {}
    for i in range(4):
        Image.fromarray(frames[i]).save(str(scene / "rgb" / ("%06d.png" % i)))
        R, t = D.random_pose(rs, K, H, W, *zr[i])
        other = {"cam_R_m2c": np.eye(3).ravel().tolist(), "cam_t_m2c": [0.0, 0.0, 900.0], "obj_id": 3 - first[i]}
        gts[str(i)] = [{"cam_R_m2c": R.ravel().tolist(), "cam_t_m2c": t.tolist(), "obj_id": first[i]}, other]
        cams[str(i)] = {"cam_K": K.ravel().tolist(), "depth_scale": 1.0}
    (scene / "scene_gt.json").write_text(json.dumps(gts))
    (scene / "scene_camera.json").write_text(json.dumps(cams))
    written = make_train_xyz.run(0, {"dataset_dir": str(tmp_path / "bop"), "skimage": "0.14"}, "lmo", batch=2, log=lambda *a: None)
    assert written == {1: 3, 2: 1}
    assert sorted(os.listdir(root / "models_xyz")) == ["norm_factor.json", "obj_000001.ply", "obj_000002.ply"]
    assert sorted(os.listdir(root / "train_xyz" / "01")) == ["000000.npy", "000001.npy", "000002.npy"]
    assert sorted(os.listdir(root / "train_xyz" / "02")) == ["000000.npy"]
    count = {1: 0, 2: 0}
    for i in range(4):
        oid = first[i]
        v, t, c = read_xyz_model(str(root / "models_xyz" / ("obj_%06d.ply" % oid)))
        sym = [0, 0, 1, 0, 0, 0] if oid == 2 else [0] * 6
        R, _ = get_sympose(np.array(gts[str(i)][0]["cam_R_m2c"]).reshape(3, 3), sym)
        cr, dr, owner, margin = X.render_xyz(v, t, c, K, R, gts[str(i)][0]["cam_t_m2c"], H, W)
        got = np.load(str(root / "train_xyz" / ("%02d" % oid) / ("%06d.npy" % count[oid])))
        count[oid] += 1
        want = X.patch(frames[i], cr, dr, X.bbox_of(dr), 0)
        assert got.shape == want.shape and got.dtype == np.uint8 and max(got.shape[:2]) <= 128
        # The driver renders on the device, the restatement here: colours agree to COLOR_TOL away from edges, so a byte may differ
        # at a centre within 1e-4 px of an edge (the colour parity's allowance) or where c * 255 + 0.5 lies within 255 * COLOR_TOL of
        # an integer, i.e. where that colour difference can move the 8-bit level; nowhere else.
        fr = cr.astype(np.float64) * 255 + 0.5
        level = (np.abs(fr - np.round(fr)) <= 255 * COLOR_TOL).any(axis=2)
        b = X.bbox_of(dr)
        allowed = (margin | level)[b[0]:b[2], b[1]:b[3]]
        differs = (got != want).any(axis=2)
        print("image %d: %s, differing pixels %d, allowed %d" % (i, got.shape, differs.sum(), allowed.sum()))
        if max(b[2] - b[0], b[3] - b[1]) <= 128:
            assert not np.any(differs & ~allowed)
        else:
            assert differs.sum() <= 4 * int(allowed.sum())      # resized: a source pixel reaches at most 2 x 2 output pixels


def test_make_train_xyz_uses_the_global_camera_for_hb(tmp_path):
    """hb / ycbv / itodd render through camera.json: a tree named hb whose per-image cam_K is deliberately wrong and whose camera.json
    is right gives the patch of the right camera."""
    import json
    from PIL import Image
    from pix2pose_amd import make_train_xyz
    from pix2pose_amd.mesh import write_ply_rgb
    from pix2pose_amd.xyz_model import read_xyz_model
    K, H, W = D.K_640, 480, 640
    root = tmp_path / "bop" / "hb"
    (root / "models").mkdir(parents=True)
    v, t = D.box_mesh([-40, -30, -15], [40, 30, 15], 3)
    write_ply_rgb(str(root / "models" / "obj_000001.ply"), v, t, np.zeros((len(v), 3), np.uint8))
    (root / "models" / "models_info.json").write_text(json.dumps({"1": {"diameter": 100.0}}))
    (root / "camera.json").write_text(json.dumps({"fx": K[0, 0], "fy": K[1, 1], "cx": K[0, 2], "cy": K[1, 2], "width": W, "height": H}))
    scene = root / "train" / "000001"
    (scene / "rgb").mkdir(parents=True)
    frame = _frames(1, H, W, 80)[0]
    Image.fromarray(frame).save(str(scene / "rgb" / "000000.png"))
    R, tt = D.random_pose(np.random.RandomState(81), K, H, W, 0.7, 1.0)
    wrong = (K * np.array([[0.5], [0.5], [1.0]])).ravel().tolist()
    (scene / "scene_gt.json").write_text(json.dumps({"0": [{"cam_R_m2c": R.ravel().tolist(), "cam_t_m2c": tt.tolist(), "obj_id": 1}]}))
    (scene / "scene_camera.json").write_text(json.dumps({"0": {"cam_K": wrong, "depth_scale": 1.0}}))
    assert make_train_xyz.run(0, {"dataset_dir": str(tmp_path / "bop"), "skimage": "0.18"}, "hb", log=lambda *a: None) == {1: 1}
    vv, tv, c = read_xyz_model(str(root / "models_xyz" / "obj_000001.ply"))
    cr, dr, owner, margin = X.render_xyz(vv, tv, c, K, R, tt, H, W)
    got = np.load(str(root / "train_xyz" / "01" / "000000.npy"))
    want = X.patch(frame, cr, dr, X.bbox_of(dr), 1)
    assert got.shape == want.shape and max(got.shape[:2]) <= 128 and want.shape[0] > 20
    fr = cr.astype(np.float64) * 255 + 0.5
    b = X.bbox_of(dr)
    allowed = (margin | (np.abs(fr - np.round(fr)) <= 255 * COLOR_TOL).any(axis=2))[b[0]:b[2], b[1]:b[3]]
    assert not np.any((got != want).any(axis=2) & ~allowed)
