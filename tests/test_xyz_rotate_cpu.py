"""CPU tests of the in-plane rotation copies' restatement (tests/xyz_rot_ref.py): skimage.transform.rotate(
resize=True) of scikit-image 0.18.3 bit for bit (recorded outputs of the real library in tests/golden/skimage_rotate018.npz, and the
live library where it imports), the quarter turns, the box and patch logic, the input tables and the driver's cfg handling."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xyz_ref as X  # noqa: E402
import xyz_rot_ref as Q  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skimage_rotate018.npz")
SIZES = ((9, 13), (17, 24), (37, 53))
ANGLES = tuple(range(30, 360, 30))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("size", SIZES)
def test_restatement_equals_recorded_skimage_018(golden, size):
    """Shapes, the float64 mask and the float32 colour at both cvals, every angle of 30 ... 330: no bit differs."""
    assert str(golden["version"]) == "0.18.3"
    key = "%dx%d" % size
    img = golden[key + "_img"].view(np.float32)
    mask = golden[key + "_mask"].view(np.float64)
    assert img.shape == size + (3,) and mask.shape == size
    for a in ANGLES:
        for tag, im, cval, bits in (("c0", img, 0, np.uint32), ("c5", img, 0.5, np.uint32), ("m", mask, 0, np.uint64)):
            want = golden["%s_a%03d_%s" % (key, a, tag)]
            got = Q.rotate(im, a, cval=cval)
            assert got.dtype == im.dtype and got.shape == want.shape, (key, a, tag, got.shape, want.shape)
            assert np.array_equal(np.ascontiguousarray(got).view(bits), want), (key, a, tag)


def test_restatement_equals_live_skimage_on_a_fresh_image():
    """Where scikit-image imports (0.17 / 0.18 only: later versions changed the warp), the same on an image no fixture holds,
    with a range that leaves cval outside it so the clip's cval rule acts."""
    skimage = pytest.importorskip("skimage")
    if tuple(int(x) for x in skimage.__version__.split(".")[:2]) not in ((0, 17), (0, 18)):
        pytest.skip("scikit-image %s is not the generation restated here" % skimage.__version__)
    from skimage.transform import rotate
    rs = np.random.RandomState(int.from_bytes(os.urandom(4), "little"))
    h, w = int(rs.randint(5, 60)), int(rs.randint(5, 60))
    img = (rs.randint(0, 256, (h, w, 3)) / 255).astype(np.float32)
    high = (np.float32(0.6) + np.float32(0.4) * img).astype(np.float32)
    mask = (rs.rand(h, w) > 0.5).astype(np.float64)
    for a in list(ANGLES) + [float(rs.uniform(1, 359))]:
        for im, cval in ((img, 0), (img, 0.5), (high, 0.5), (high, 0), (mask, 0)):
            want = rotate(im, a, resize=True, cval=cval)
            got = Q.rotate(im, a, cval=cval)
            bits = np.uint32 if im.dtype == np.float32 else np.uint64
            assert got.shape == want.shape and got.dtype == want.dtype
            assert np.array_equal(np.ascontiguousarray(got).view(bits), np.ascontiguousarray(want).view(bits)), (h, w, a, cval)


def test_runtime_matrix_is_the_restatements():
    """The host code of the package forms the matrix and shape that the restatement (held to tform.params through the warps above)
    forms: same bits."""
    from pix2pose_amd.runtime import skimage_rotate_matrix
    for (h, w) in SIZES + ((480, 640), (150, 200)):
        for a in ANGLES + (10, 45.5):
            m1, s1 = skimage_rotate_matrix(h, w, a)
            m2, s2 = Q.rotate_matrix(h, w, a)
            assert s1 == s2 and np.array_equal(m1.view(np.uint64), m2.view(np.uint64))
            assert m1[2].tolist() == [0, 0, 1]


def test_quarter_turns_are_permutations():
    """90, 180 and 270 degrees of a small image move pixels and change none (cos and sin are 6e-17 or 1.2e-16 off, never enough to
    reach a neighbour's weight in float32; the float64 mask may mix 1e-16 of a neighbour in, so it is held to 1e-12)."""
    rs = np.random.RandomState(5)
    img = (rs.randint(0, 256, (6, 9, 3)) / 255).astype(np.float32)
    mask = (rs.rand(6, 9) > 0.5).astype(np.float64)
    for a, k in ((90, 1), (180, 2), (270, 3)):
        got = Q.rotate(img, a, cval=0.5)
        assert got.shape == np.rot90(img, k).shape
        assert np.array_equal(got, np.rot90(img, k)), a
        gm = Q.rotate(mask, a)
        assert gm.shape == np.rot90(mask, k).shape and np.abs(gm - np.rot90(mask, k)).max() < 1e-12


def test_box_and_patch_on_a_hand_made_case():
    """5 x 7 frame, a 2 x 3 block drawn, turned by 180 degrees: the rotated mask is the block mirrored through the centre; the box is
    [min v, min u, max v, max u] with the max inclusive, the patch leaves the last row and column out, holds the frame with grey
    where nothing is drawn and the colour through the read-back table."""
    H, W = 5, 7
    depth = np.zeros((H, W), np.float32)
    depth[1:3, 2:5] = 1.0
    rs = np.random.RandomState(6)
    rgb = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    color = np.zeros((H, W, 3), np.float32)
    color[1:3, 2:5] = rs.rand(2, 3, 3).astype(np.float32)
    m = Q.rotate((depth > 0).astype(np.float64), 180)
    box = Q.box_of_mask(m)
    # rows 1..2 -> 4-1..4-2 = 2..3, columns 2..4 -> 6-4..6-2 = 2..4 (values within 1e-15 of 1 there, tiny positives may ring around)
    core = np.argwhere(m > 0.5)
    assert core.min(0).tolist() == [2, 2] and core.max(0).tolist() == [3, 4]
    assert box[0] <= 2 and box[1] <= 2 and box[2] >= 3 and box[3] >= 4
    got = Q.rotated_unresized(rgb, color, depth, 180)
    assert got.shape == (box[2] - box[0], box[3] - box[1], 6) and got.dtype == np.uint8
    grey = np.array(rgb)
    grey[depth == 0] = 128
    want_rgb = np.rot90(grey, 2)
    want_xyz = np.rot90(X.quantise(color), 2)
    pad_r, pad_c = (m.shape[0] - H) // 2, (m.shape[1] - W) // 2
    assert m.shape == (H, W) and pad_r == 0 and pad_c == 0
    sl = (slice(box[0], box[2]), slice(box[1], box[3]))
    # a quarter-turn multiple keeps every value's float32 (test above), so times 255 and truncation give xyz_ref's bytes -- except the
    # frame's bytes q with float32(q / 255.0) * 255 below q, which the reference's rotation copies do store one lower
    rgb_tab, xyz_tab = Q.input_tables()
    assert np.array_equal(got[:, :, :3], (rgb_tab[want_rgb] * np.float32(255)).astype(np.uint8)[sl])
    assert np.array_equal(got[:, :, 3:], (xyz_tab[Q.levels(np.rot90(color, 2))] * np.float32(255)).astype(np.uint8)[sl])
    assert np.abs(got[:, :, 3:].astype(int) - want_xyz[sl].astype(int)).max() <= 1
    # an empty render has no box; a one-pixel mask has a zero-sided one at a quarter turn
    assert Q.rotated_unresized(rgb, color, np.zeros((H, W), np.float32), 30) is None
    one = np.zeros((H, W), np.float32)
    one[2, 3] = 1.0
    b1 = Q.box_of_mask(Q.rotate((one > 0).astype(np.float64), 30))
    assert b1 is not None and b1[2] - b1[0] >= 1 and b1[3] - b1[1] >= 1          # bilinear spread: at least 2 x 2 positive


def test_patch_above_128_is_resized_like_the_unrotated_one():
    rs = np.random.RandomState(7)
    data = rs.randint(0, 256, (150, 90, 6)).astype(np.uint8)
    out = Q.resize_patch(data, 1)
    assert out.shape == X.patch_shape(150, 90) + (6,) == (128, 77, 6)
    small = data[:100, :60]
    assert Q.resize_patch(small, 1) is small


def test_input_tables_follow_their_definitions():
    rgb, xyz = Q.input_tables()
    from pix2pose_amd.runtime import rotate_input_tables
    r2, x2 = rotate_input_tables()
    assert rgb.dtype == xyz.dtype == r2.dtype == x2.dtype == np.float32
    assert np.array_equal(rgb.view(np.uint32), r2.view(np.uint32)) and np.array_equal(xyz.view(np.uint32), x2.view(np.uint32))
    for q in range(256):
        assert rgb[q] == np.float32(q / 255.0)
        back = np.float32(np.float32(np.float32(q) / np.float32(255)) * np.float32(255))      # get_rendering's img_r
        assert xyz[q] == np.float32(back / np.float32(255))
    # as arrays, the way the reference computes them
    frame = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal((frame / 255).astype(np.float32), rgb[frame])
    img_r = (np.arange(256, dtype=np.float32) / np.float32(255)).reshape(16, 16) * 255
    assert img_r.dtype == np.float32 and np.array_equal((img_r / 255).astype(np.float32).ravel(), xyz)
    assert rgb[128] == np.float32(128 / 255) and xyz[0] == 0 and rgb[255] == 1 and xyz.max() <= 1


def test_driver_cfg_handling(tmp_path):
    """augment_inplane: absent or 0 -> no angles; 30 with skimage 0.18 -> 30 ... 330; with another generation ValueError, raised by
    run() before models_xyz or train_xyz exist."""
    from pix2pose_amd import make_train_xyz as M
    assert M.inplane_angles({}, 0) == [] and M.inplane_angles({"augment_inplane": 0}, 2) == []
    assert M.inplane_angles({"augment_inplane": 30}, 1) == list(range(30, 360, 30))
    assert M.inplane_angles({"augment_inplane": 100}, 1) == [100, 200, 300]
    for bad in (-30, 360, 12.5, "30", True):
        with pytest.raises(ValueError, match="augment_inplane"):
            M.inplane_angles({"augment_inplane": bad}, 1)
    root = tmp_path / "bop" / "lmo"
    (root / "models").mkdir(parents=True)
    (root / "models" / "models_info.json").write_text(json.dumps({}))
    for ver in ("0.14", "0.15", "0.16"):
        with pytest.raises(ValueError, match="0.17"):
            M.run(0, {"dataset_dir": str(tmp_path / "bop"), "skimage": ver, "augment_inplane": 30}, "lmo", log=lambda *a: None)
    assert sorted(os.listdir(root)) == ["models"]
