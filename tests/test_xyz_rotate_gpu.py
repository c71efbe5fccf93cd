"""GPU tests of the in-plane rotation copies of the training patches (csrc/xyz_patch.hip: p2p_xyz_rotate_patch_batch,
runtime.xyz_rotate_patch_batch, make_train_xyz cfg augment_inplane): device patches against the restatement
tests/xyz_rot_ref.py (held to the real scikit-image 0.18.3 by tests/test_xyz_rotate_cpu.py) byte for byte, shape included."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref as D  # noqa: E402
import xyz_ref as X  # noqa: E402
import xyz_rot_ref as Q  # noqa: E402

pytestmark = pytest.mark.gpu

ANGLES = list(range(30, 360, 30))
GEN = 1                                   # runtime.RESIZE_GENERATIONS: scikit-image 0.17 / 0.18
CAM_64x48 = (np.array([[70.0, 2.0, 30.0], [0.0, 55.0, 22.0], [0.0, 0.0, 1.0]]), 48, 64)


@pytest.fixture(scope="module")
def ctx():
    from pix2pose_amd.runtime import Context
    c = Context(0, max_batch=8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def box(ctx):
    from pix2pose_amd.runtime import Mesh
    from pix2pose_amd.xyz_model import xyz_colors
    v, t = D.box_mesh([-40, -30, -15], [40, 30, 15], 3)
    m = Mesh(ctx, v, t)
    m.set_colors(xyz_colors(v)[0])
    return m


def _job(R, t, K):
    return {"mesh": 0, "camK": K, "R": R, "t": t}


def _frames(n, H, W, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n)]


def _render(ctx, box, jobs, H, W):
    from pix2pose_amd.runtime import render_xyz_batch
    return render_xyz_batch(ctx, [box], jobs, H, W)


def _check(got, frame, color, depth, angles, gen=GEN):
    """-> number of patches compared (None entries agree as None)."""
    want = Q.augment_inplane(frame, color, depth, angles, gen)
    assert len(got) == len(want) == len(angles)
    n = 0
    for a, g, w in zip(angles, got, want):
        if w is None:
            assert g is None, a
            continue
        assert g is not None and g.dtype == np.uint8 and g.shape == w.shape, (a, None if g is None else g.shape, w.shape)
        diff = g.astype(int) - w.astype(int)
        print("angle %s: %s, differing bytes %d (max %d)" % (a, w.shape, (diff != 0).sum(), np.abs(diff).max()))
        assert np.array_equal(g, w), a
        n += 1
    return n


@pytest.mark.parametrize("cam", [D.CAMERAS[3], CAM_64x48], ids=["53x37", "64x48"])
def test_all_angles_equal_the_restatement(ctx, box, cam):
    """A box mesh under a skewed camera, every angle of 30 ... 330."""
    from pix2pose_amd.runtime import xyz_rotate_patch_batch
    K, H, W = cam
    jobs = [_job(D.rot(0, 25) @ D.rot(1, -35) @ D.rot(2, 10), [25.0, -8.0, 230.0], K)]
    frames = _frames(1, H, W, 90)
    color, depth, bbox = _render(ctx, box, jobs, H, W)
    assert (depth[0] > 0).sum() > 60 and bbox[0][0] > 0 and bbox[0][1] > 0 and bbox[0][2] < H - 1 and bbox[0][3] < W - 1
    got = xyz_rotate_patch_batch(ctx, frames, color, depth, [ANGLES], GEN)
    assert _check(got[0], frames[0], color[0], depth[0], ANGLES) == 11


def test_object_cut_by_the_border_has_cval_inside_the_box(ctx, box):
    """The object leaves the frame on the left and at the top: the rotated box holds pixels whose four taps all lie outside the frame,
    where the frame half is cval 0.5 and the colour half cval 0."""
    from pix2pose_amd.runtime import xyz_rotate_patch_batch
    K, H, W = D.CAMERAS[3]
    jobs = [_job(D.rot(0, 20) @ D.rot(2, 40), [-45.0, -60.0, 160.0], K)]
    frames = _frames(1, H, W, 91)
    color, depth, bbox = _render(ctx, box, jobs, H, W)
    assert bbox[0][0] == 0 and bbox[0][1] == 0 and (depth[0] > 0).sum() > 60
    got = xyz_rotate_patch_batch(ctx, frames, color, depth, [ANGLES], GEN)
    assert _check(got[0], frames[0], color[0], depth[0], ANGLES) == 11
    # rotate(ones, cval=0) is exactly 0 where all four taps are outside the frame: such pixels lie inside the rotated boxes, and
    # the patch holds [127] * 3 (float32(0.5) * 255 truncated) + [0] * 3 there
    n_cval = 0
    for a, p in zip(ANGLES, got[0]):
        b = Q.box_of_mask(Q.rotate((depth[0] > 0).astype(np.float64), a))
        outside = Q.rotate(np.ones((H, W)), a, cval=0)[b[0]:b[2], b[1]:b[3]] == 0
        assert np.all(p[outside] == [127, 127, 127, 0, 0, 0])
        n_cval += int(outside.sum())
    assert n_cval > 0


def _weights_agree(n_in, n_out):
    """The Gaussian weights of one resized axis by libm's exp (the library) and by numpy's exp (the restatement's scipy): True when
    they are the same doubles, so that no allowance is needed."""
    sigma = (n_in / n_out - 1) / 2
    r = int(4.0 * sigma + 0.5) if sigma > 0 else 0
    if r <= 0:
        return True
    c = -0.5 / (sigma * sigma)
    x = np.arange(-r, r + 1)
    return np.array_equal(np.exp(c * x ** 2), np.array([math.exp(c * float(k * k)) for k in x]))


RESIZE_ANGLES = [30, 60, 120, 210, 300, 330]


def test_rotated_box_above_128_px_is_resized(ctx, box):
    """200 x 150 frame, the object fills most of it: every rotated box exceeds 128 px and goes through the resize stage.  The two
    weight computations are asserted equal for every shape that occurs, and nothing is exempted."""
    from pix2pose_amd.runtime import xyz_rotate_patch_batch
    K, H, W = np.array([[260.0, 1.5, 98.0], [0.0, 255.0, 77.0], [0.0, 0.0, 1.0]]), 150, 200
    jobs = [_job(D.rot(0, 25) @ D.rot(1, -35) @ D.rot(2, 10), [0.0, 0.0, 190.0], K)]
    frames = _frames(1, H, W, 92)
    color, depth, bbox = _render(ctx, box, jobs, H, W)
    got = xyz_rotate_patch_batch(ctx, frames, color, depth, [RESIZE_ANGLES], GEN)
    for a, g in zip(RESIZE_ANGLES, got[0]):
        raw = Q.rotated_unresized(frames[0], color[0], depth[0], a)
        h, w = raw.shape[:2]
        assert max(h, w) > 128, (a, h, w)
        oh, ow = X.patch_shape(h, w)
        assert _weights_agree(h, oh) and _weights_agree(w, ow), (a, h, w)
        assert g.shape == (oh, ow, 6) and max(oh, ow) == 128
    assert _check(got[0], frames[0], color[0], depth[0], RESIZE_ANGLES) == len(RESIZE_ANGLES)


def _batch(ctx, box, n, seed):
    K, H, W = D.CAMERAS[3]
    rs = np.random.RandomState(seed)
    jobs = [_job(*D.random_pose(rs, K, H, W, 0.15, 0.3), K) for _ in range(n)]
    frames = _frames(n, H, W, seed + 1)
    color, depth, bbox = _render(ctx, box, jobs, H, W)
    angles = [ANGLES[:(k * 5) % 12] for k in range(n)]                 # 0, 5, 10, 3, 8, 1, ... angles: lists of different lengths
    return frames, color, depth, angles


@pytest.mark.parametrize("n", [1, 3, 33])
def test_batches_with_angle_lists_of_different_lengths(ctx, box, n):
    from pix2pose_amd.runtime import xyz_rotate_patch_batch
    frames, color, depth, angles = _batch(ctx, box, n, 100 + n)
    if n == 1:
        angles = [ANGLES[:4]]
    got = xyz_rotate_patch_batch(ctx, frames, color, depth, angles, GEN)
    assert [len(g) for g in got] == [len(a) for a in angles]
    done = sum(_check(got[k], frames[k], color[k], depth[k], angles[k]) for k in range(n))
    assert done >= (2 if n == 1 else n)


def test_a_job_alone_and_in_a_batch_gives_identical_bytes(ctx, box):
    from pix2pose_amd.runtime import xyz_rotate_patch_batch
    frames, color, depth, angles = _batch(ctx, box, 7, 120)
    got = xyz_rotate_patch_batch(ctx, frames, color, depth, angles, GEN)
    for k in (1, 4, 6):
        alone = xyz_rotate_patch_batch(ctx, frames[k:k + 1], color[k:k + 1], depth[k:k + 1], angles[k:k + 1], GEN)[0]
        assert len(alone) == len(got[k]) > 0
        for p, q in zip(alone, got[k]):
            assert (p is None and q is None) or (p.shape == q.shape and np.array_equal(p, q))


def test_empty_render_gives_none(ctx, box):
    from pix2pose_amd.runtime import xyz_rotate_patch_batch
    K, H, W = D.CAMERAS[3]
    jobs = [_job(D.rot(2, 5), [3000.0, 0.0, 300.0], K), _job(np.eye(3), [0.0, 0.0, 200.0], K)]
    frames = _frames(2, H, W, 93)
    color, depth, bbox = _render(ctx, box, jobs, H, W)
    assert not depth[0].any() and depth[1].any()
    got = xyz_rotate_patch_batch(ctx, frames, color, depth, [[30, 90], [30]], GEN)
    assert got[0] == [None, None] and got[1][0] is not None
    assert Q.augment_inplane(frames[0], color[0], depth[0], [30, 90]) == [None, None]


def test_argument_errors(ctx, box):
    from pix2pose_amd import _lib
    from pix2pose_amd.runtime import rotate_input_tables, xyz_rotate_patch_batch
    K, H, W = D.CAMERAS[3]
    jobs = [_job(np.eye(3), [0.0, 0.0, 200.0], K)]
    frames = _frames(1, H, W, 94)
    color, depth, bbox = _render(ctx, box, jobs, H, W)
    for gen in (0, 2, 3):
        with pytest.raises(_lib.P2PError, match="generation"):
            xyz_rotate_patch_batch(ctx, frames, color, depth, [[30]], gen)
    with pytest.raises(_lib.P2PError, match="angle list"):
        xyz_rotate_patch_batch(ctx, frames, color, depth, [[30, float("nan")]], GEN)
    with pytest.raises(ValueError, match="one size"):
        xyz_rotate_patch_batch(ctx, frames, color, depth[:, :-1], [[30]], GEN)
    L = _lib.lib()
    rgb_tab, xyz_tab = rotate_input_tables()
    rp = (_lib.C.c_void_p * 1)(frames[0].ctypes.data)
    cnt = np.array([-1], np.int32)
    mats, shp = np.zeros((1, 6)), np.array([[H, W]], np.int32)
    out, shapes = np.zeros((1, 128, 128, 6), np.uint8), np.zeros((1, 2), np.int32)

    def call(cnt, mats, shp, h=H, w=W, tab=rgb_tab):
        return L.p2p_xyz_rotate_patch_batch(ctx.handle, rp, color.ctypes.data, depth.ctypes.data, 1, h, w, cnt.ctypes.data, mats.ctypes.data,
                                            shp.ctypes.data, tab.ctypes.data, xyz_tab.ctypes.data, GEN, out.ctypes.data, shapes.ctypes.data)
    assert call(cnt, mats, shp) == -1 and b"angle list" in L.p2p_last_error()
    cnt[0] = 1
    assert call(cnt, mats, np.array([[H, 4 * (H + W)]], np.int32)) == -1 and b"angle list" in L.p2p_last_error()
    assert call(cnt, mats, shp, h=0) == -1 and b"image size" in L.p2p_last_error()
    assert call(cnt, mats, shp, tab=rgb_tab + np.float32(1)) == -1 and b"table" in L.p2p_last_error()
    assert L.p2p_xyz_rotate_patch_batch(ctx.handle, None, None, None, 1, H, W, None, None, None, None, None, GEN, None, None) == -1
    assert xyz_rotate_patch_batch(ctx, frames, color, depth, [[30]], GEN)[0][0] is not None


# ---- driver ----------------------------------------------------------------------------------------------------------------

def _tree(tmp_path, name, poses, sym_obj2=True):
    """A synthetic BOP tree with objects 1 (L shape) and 2 (box, continuous symmetry about z); image i shows object first[i]."""
    import json
    from PIL import Image
    from pix2pose_amd.mesh import write_ply_rgb
    K, H, W = D.K_640, 480, 640
    root = tmp_path / "bop" / name
    (root / "models").mkdir(parents=True)
    geo = {1: D.l_mesh(4), 2: D.box_mesh([-40, -30, -15], [40, 30, 15], 3)}
    for oid, (v, t) in geo.items():
        write_ply_rgb(str(root / "models" / ("obj_%06d.ply" % oid)), v, t, np.zeros((len(v), 3), np.uint8))
    info = {"1": {"diameter": 100.0}, "2": {"diameter": 100.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}
    (root / "models" / "models_info.json").write_text(json.dumps(info))
    (root / "camera.json").write_text(json.dumps({"fx": K[0, 0], "fy": K[1, 1], "cx": K[0, 2], "cy": K[1, 2], "width": W, "height": H}))
    scene = root / "train" / "000001"
    (scene / "rgb").mkdir(parents=True)
    frames, gts, cams = _frames(len(poses), H, W, 95), {}, {}
    for i, (oid, R, t) in enumerate(poses):
        Image.fromarray(frames[i]).save(str(scene / "rgb" / ("%06d.png" % i)))
        gts[str(i)] = [{"cam_R_m2c": np.asarray(R).ravel().tolist(), "cam_t_m2c": list(t), "obj_id": oid}]
        cams[str(i)] = {"cam_K": K.ravel().tolist(), "depth_scale": 1.0}
    (scene / "scene_gt.json").write_text(json.dumps(gts))
    (scene / "scene_camera.json").write_text(json.dumps(cams))
    return root, frames, K, H, W


def test_driver_writes_twelve_files_per_image_and_none_for_a_locked_pose(tmp_path):
    """lmo tree, augment_inplane = 30: object 1's two images get <n>.npy and <n>_030 ... <n>_330.npy, each equal to the restatement
    on the device's render; object 2 is seen along its symmetry axis (axis along the camera z: get_sympose locks the rotation), so it
    gets its <n>.npy alone.  With the default cfg the same tree gets no copies."""
    from pix2pose_amd import make_train_xyz
    from pix2pose_amd.runtime import Context, Mesh, render_xyz_batch
    from pix2pose_amd.xyz_model import get_sympose
    poses = [(1, D.rot(0, 30) @ D.rot(1, 20), [20.0, -10.0, 800.0]), (2, D.rot(2, 25), [0.0, 0.0, 700.0]),
             (1, D.rot(1, -50) @ D.rot(2, 70), [-60.0, 40.0, 900.0])]
    root, frames, K, H, W = _tree(tmp_path, "lmo", poses)
    assert get_sympose(poses[1][1], [0, 0, 1, 0, 0, 0])[1] is True
    cfg = {"dataset_dir": str(tmp_path / "bop"), "skimage": "0.18", "augment_inplane": 30}
    assert make_train_xyz.run(0, cfg, "lmo", batch=2, log=lambda *a: None) == {1: 2, 2: 1}
    names = ["%06d.npy" % n for n in range(2)] + ["%06d_%03d.npy" % (n, r) for n in range(2) for r in ANGLES]
    assert sorted(os.listdir(root / "train_xyz" / "01")) == sorted(names) and len(names) == 24
    assert sorted(os.listdir(root / "train_xyz" / "02")) == ["000000.npy"]
    # the files hold the restatement's patches of the device's render
    c = Context(0, max_batch=8)
    try:
        mesh = Mesh.from_xyz_ply(c, str(root / "models_xyz" / "obj_000001.ply"))
        color, depth, bbox = render_xyz_batch(c, [mesh], [_job(poses[2][1], poses[2][2], K)], H, W)
        mesh.close()
    finally:
        c.close()
    got = [np.load(str(root / "train_xyz" / "01" / ("000001_%03d.npy" % r))) for r in (30, 180, 330)]
    assert _check(got, frames[2], color[0], depth[0], [30, 180, 330]) == 3
    # default cfg: today's output, no copies
    root2, *_ = _tree(tmp_path / "plain", "lmo", poses)
    make_train_xyz.run(0, {"dataset_dir": str(tmp_path / "plain" / "bop"), "skimage": "0.18"}, "lmo", batch=2, log=lambda *a: None)
    assert sorted(os.listdir(root2 / "train_xyz" / "01")) == ["000000.npy", "000001.npy"]
    assert np.array_equal(np.load(str(root2 / "train_xyz" / "01" / "000001.npy")), np.load(str(root / "train_xyz" / "01" / "000001.npy")))
