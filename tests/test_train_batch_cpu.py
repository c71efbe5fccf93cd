"""CPU tests of the training-batch path: the restatement tests/train_ref.py against the recorded outputs of
the reference's own get_patch_pair under scikit-image 0.18.3 (tests/golden/reference_train_batch*.npz), runtime.train_draws against
the recorded draw stream, the dilation identity the kernels rely on, and the binding's view of the new entry point."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ref as T  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SAMPLES = T.load_samples(GOLDEN)


def draw_record(s):
    from pix2pose_amd import runtime
    random.seed(s["seed"])
    return runtime.train_draws(random, s["patch"].shape, s["back"].shape, s["batch_count"])


def test_fixture_covers_the_cases():
    names = [s["name"] for s in SAMPLES]
    assert len(names) == 10 and sorted(s["imsize"] for s in SAMPLES) == [64] * 8 + [128] * 2
    assert {s["batch_count"] % 2 for s in SAMPLES} == {0, 1}
    by = dict(zip(names, SAMPLES))
    assert by["even_128x90_7ch"]["patch"].shape == (128, 90, 7) and by["odd_nonsquare_37x61"]["patch"].shape == (37, 61, 6)
    assert by["grey_background"]["back"].ndim == 2
    assert by["enlarged_one_axis"]["back"].shape[:2] == (100, 180) and by["enlarged_one_axis"]["ints"]["frame_h"] == 120
    assert by["clipped_top_left"]["ints"]["shift_v"] > 0 and by["clipped_top_left"]["ints"]["shift_u"] > 0
    assert by["clipped_bottom_right"]["ints"]["shift_v_max"] < 0 and by["clipped_bottom_right"]["ints"]["shift_u_max"] < 0
    assert draw_record(by["sigmas_radius_0"])["sigma_edge"] < 0.125 and draw_record(by["sigmas_radius_0"])["sigma_blur"] < 0.125
    assert draw_record(by["sigmas_near_2"])["sigma_edge"] > 1.8 and draw_record(by["sigmas_near_2"])["sigma_blur"] > 1.8
    # a negative start of the first rectangle: Python's slice counts it from the frame's end
    s = by["negative_rectangle_start"]
    r = draw_record(s)
    assert r["rect"][0][0] > s["ints"]["frame_h"] - 10 or r["rect"][0] == [0, 0, 0, 0]
    assert draw_record(by["second_rectangle_h_aug_0"])["rect"][1] == [0, 0, 0, 0]


@pytest.mark.parametrize("s", SAMPLES, ids=[s["name"] for s in SAMPLES])
def test_train_draws_consumes_the_recorded_stream(s):
    """The seeded `random` stream becomes exactly the recorded draws (bit for bit, nothing more and nothing less consumed) and the
    integers the reference derived from them."""
    r = draw_record(s)
    assert np.array_equal(np.array(r["draws"]).view(np.uint64), np.array(s["draws"]).view(np.uint64))
    assert len(r["draws"]) == (23 if s["batch_count"] % 2 == 0 else 14)
    want = s["ints"]
    for f in ("v_ref", "u_ref", "v1", "v2", "u1", "u2", "shift_v", "shift_u", "side"):
        assert r[f] == want[f], f
    assert r["frame"] == (want["frame_h"], want["frame_w"])
    assert r["side"] - r["shift_v"] - (r["v2"] - r["v1"]) == -want["shift_v_max"]
    assert r["side"] - r["shift_u"] - (r["u2"] - r["u1"]) == -want["shift_u_max"]
    assert np.float64(r["angle"]).view(np.uint64) == np.float64(s["angle"]).view(np.uint64)
    assert r["even"] == (1 if s["batch_count"] % 2 == 0 else 0)


@pytest.mark.parametrize("s", SAMPLES, ids=[s["name"] for s in SAMPLES])
def test_restatement_equals_the_recorded_reference(s):
    """max |difference| <= 1e-9 on src, tgt and mask, no pixel excepted (the fixture's quantum is 7e-12)."""
    src, tgt, mask = T.get_patch_pair(s["patch"], s["back"], draw_record(s), s["imsize"])
    for name, got, want in (("src", src, s["src"]), ("tgt", tgt, s["tgt"]), ("mask", mask, s["mask"])):
        assert got.shape == want.shape and got.dtype == np.float64
        d = float(np.abs(got - want).max())
        print(s["name"], name, "max |d| = %.3g" % d)
        assert d <= 1e-9, (s["name"], name, d)


def test_recorded_margin_of_the_radius_threshold():
    """No window pixel of an even-batch sample has |radius - 0.3| < 1e-4 (the maker's assertion, seen from the restatement)."""
    for s in SAMPLES:
        if s["batch_count"] % 2 == 0:
            assert T.radius_margin(s["patch"], draw_record(s)) >= 1e-4 - 1e-12, s["name"]


def test_thresholded_gaussian_is_a_square_dilation():
    """gaussian_filter(m, sigma, mode='nearest') > 0 == dilation by the square of radius int(4 sigma + 0.5), sigma over (0, 2]."""
    from scipy import ndimage as ndi
    rs = np.random.RandomState(3)
    sigmas = list(np.linspace(0.02, 2.0, 34)) + [0.1249, 0.125, 0.1251, 0.3749, 0.375, 0.62, 1.999]
    for i, sigma in enumerate(sigmas):
        m = rs.rand(37, 41) < (0.01 if i % 2 else 0.2)
        m[0, 0] = m[-1, 17] = True                      # on the border, where mode='nearest' repeats them
        r = int(4.0 * sigma + 0.5)
        want = ndi.binary_dilation(m, structure=np.ones((2 * r + 1, 2 * r + 1), bool)) if r > 0 else m
        got = ndi.gaussian_filter(m.astype(float), sigma, mode="nearest", truncate=4.0) > 0
        assert np.array_equal(got, want), sigma


def test_rotate_matrix_is_the_identity_at_angle_0_and_a_rotation_about_the_centre():
    from pix2pose_amd import runtime
    assert np.array_equal(runtime.train_rotate_matrix(128, 0.0), [1, 0, 0, 0, 1, 0])
    m = runtime.train_rotate_matrix(90, 10.0).reshape(2, 3)
    c = 90 / 2 - 0.5
    assert np.allclose(m @ [c, c, 1], [c, c], atol=1e-12)


def test_train_colours_records_are_in_range_and_repeat_with_the_seed():
    from pix2pose_amd import runtime
    a = runtime.train_colours(np.random.default_rng(4), 200)
    b = runtime.train_colours(np.random.default_rng(4), 200)
    assert a == b
    assert all(sorted(r["order"]) == list(range(8)) for r in a)
    assert all(-15 <= v <= 15 for r in a for v in r["add"]) and all(0.8 <= r["contrast"] <= 1.3 for r in a)
    assert all(0 <= r["blur_sigma"] <= 0.5 for r in a) and {r["noise_scale"] for r in a} == {0.0, 10.0}
    assert any(len(set(r["mul"])) == 3 for r in a) and any(len(set(r["mul"])) == 1 for r in a)
    assert [r["sample"] for r in a] == list(range(200))


def test_entry_point_is_exported_and_struct_sizes_match():
    from pix2pose_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "p2p_train_batch")
    assert L.p2p_train_sizeof(0) == C.sizeof(_lib.TrainDraw) and L.p2p_train_sizeof(1) == C.sizeof(_lib.TrainColour)
    assert L.p2p_train_sizeof(2) == -1
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "p2p_mi355.h")).read()
    assert "P2P_TRAIN_MAX_PATCH %d" % _lib.TRAIN_MAX_PATCH in hdr and "P2P_TRAIN_MAX_WINDOW %d" % _lib.TRAIN_MAX_WINDOW in hdr


def test_train_patch_batch_rejects_mismatched_lists_before_the_library():
    from pix2pose_amd import runtime
    with pytest.raises(ValueError):
        runtime.train_patch_batch(None, [np.zeros((4, 4, 6), np.uint8)], [], [])
