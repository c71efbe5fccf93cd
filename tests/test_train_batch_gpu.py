"""GPU tests of the training-batch path (csrc/train_batch.hip: p2p_train_batch, runtime.train_patch_batch, pix2pose_amd.data_io;
DESIGN.md section 8.5): device batches against the recorded outputs of the reference's own get_patch_pair / generator() under
scikit-image 0.18.3, the colour stage against its numpy application, its noise generator's statistics, and the per-sample status.

The bar against the recordings is the project's bar for generator tensors in [-1, 1]: 1e-4.  The issue allows 0.1 % of a sample's
pixels, each within 2 pixels of a mask or rectangle edge, to exceed it; the tests below allow none, which asks no less."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4


@pytest.fixture(scope="module")
def ctx():
    from pix2pose_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def samples():
    from pix2pose_amd import runtime
    out = T.load_samples(GOLDEN)
    for s in out:
        random.seed(s["seed"])
        s["rec"] = runtime.train_draws(random, s["patch"].shape, s["back"].shape, s["batch_count"])
    return out


def run(ctx, group, imsize, colours=None, **kw):
    from pix2pose_amd.runtime import train_patch_batch
    return train_patch_batch(ctx, [s["patch"] for s in group], [s["back"] for s in group], [s["rec"] for s in group], colours, imsize, **kw)


@pytest.fixture(scope="module")
def batched(ctx, samples):
    """Every fixture sample through ONE call per output size (a call has one imsize): mixed shapes and parities together."""
    out = {}
    for imsize in (64, 128):
        group = [s for s in samples if s["imsize"] == imsize]
        src, tgt, mask = run(ctx, group, imsize)
        for k, s in enumerate(group):
            out[s["name"]] = (src[k], tgt[k], mask[k])
    return out


def test_fixture_samples_in_one_batch_match_the_reference(samples, batched):
    worst, over = 0.0, 0
    for s in samples:
        for name, got, want in zip(("src", "tgt", "mask"), batched[s["name"]], (s["src"], s["tgt"], s["mask"])):
            assert got.shape == want.shape and got.dtype == np.float32
            d = np.abs(got.astype(np.float64) - want)
            print("%-28s %-4s max |d| = %.3g, pixels over %g: %d" % (s["name"], name, d.max(), TOL, int((d > TOL).sum())))
            worst, over = max(worst, float(d.max())), over + int((d > TOL).sum())
    print("all samples: max |d| = %.3g, pixels over the bar: %d" % (worst, over))
    assert over == 0 and worst <= TOL


def test_one_by_one_equals_the_batch_bit_for_bit(ctx, samples, batched):
    for s in samples:
        alone = run(ctx, [s], s["imsize"])
        for a, b in zip(alone, batched[s["name"]]):
            assert np.array_equal(a[0].view(np.uint32), b.view(np.uint32)), s["name"]


def test_device_outputs_are_torch_tensors_with_the_same_bits(ctx, samples, batched):
    import torch
    group = [s for s in samples if s["imsize"] == 64][:3]
    src, tgt, mask = run(ctx, group, 64, device=True)
    assert isinstance(src, torch.Tensor) and src.is_cuda and src.shape == (3, 64, 64, 3) and mask.shape == (3, 64, 64)
    for k, s in enumerate(group):
        for a, b in zip((src, tgt, mask), batched[s["name"]]):
            assert np.array_equal(a[k].cpu().numpy().view(np.uint32), b.view(np.uint32)), s["name"]


def test_generator_reproduces_the_recorded_batches(ctx, tmp_path):
    """data_generator.generator() with the fixture's seed, file lists and colour=False: the reference's first two batches (batch_count 0
    and 1, a wrap-around of the four views in between), its shapes and its constant batch_tgt_disc."""
    from pix2pose_amd.data_io import data_generator
    g = np.load(os.path.join(GOLDEN, "reference_train_generator.npz"))
    data_dir, back_dir = tmp_path / "data", tmp_path / "back"
    data_dir.mkdir()
    back_dir.mkdir()
    datafiles, backfiles = [str(f) for f in g["datafiles"]], [str(f) for f in g["backfiles"]]
    for k, fn in enumerate(datafiles):
        np.save(str(data_dir / fn), g["patch_%d" % k])
    for k, fn in enumerate(backfiles):
        np.save(str(back_dir / fn), g["back_%d" % k])
    gen = data_generator(str(data_dir), str(back_dir), batch_size=3, imsize=64, ctx=ctx, colour=False)
    assert sorted(gen.datafiles) == sorted(datafiles) and gen.n_data == 4 and gen.n_background == 3
    gen.datafiles, gen.backfiles = datafiles, backfiles          # os.listdir's order is the file system's: take the recorded one
    random.seed(int(g["seed"]))
    np.random.seed(int(g["seed"]))
    it = gen.generator()
    scale = float(g["scale"])
    for k in range(2):
        src, tgt, disc, prob = next(it)
        assert src.shape == (3, 64, 64, 3) and tgt.shape == (3, 64, 64, 3) and disc.shape == (3,) and prob.shape == (3, 64, 64, 1)
        assert np.array_equal(disc, g["disc_%d" % k]) and np.all(disc == 1)
        for name, got, want in (("src", src, g["src_%d" % k]), ("tgt", tgt, g["tgt_%d" % k]), ("prob", prob, g["prob_%d" % k])):
            d = np.abs(got.astype(np.float64) - want / scale)
            print("batch %d %-4s max |d| = %.3g, pixels over %g: %d" % (k, name, d.max(), TOL, int((d > TOL).sum())))
            assert d.max() <= TOL
    gen.gan = False
    assert len(next(it)) == 2
    one = gen.get_patch_pair(0, 1)
    assert one[0].shape == (64, 64, 3) and one[1].shape == (64, 64, 3) and one[2].shape == (64, 64)


def test_colour_stage_without_noise_matches_its_numpy_application(ctx, samples):
    """Eight samples with drawn orders and parameters (noise off): within 1e-5 of the 0 .. 1 image values, i.e. 2e-5 of src."""
    from pix2pose_amd import runtime
    group = [s for s in samples if s["imsize"] == 64]
    assert len(group) == 8
    colours = runtime.train_colours(np.random.default_rng(11), 8)
    for c in colours:
        c["noise_scale"] = 0.0
    assert len({tuple(c["order"]) for c in colours}) == 8 and any(int(4 * c["blur_sigma"] + 0.5) > 0 for c in colours)
    src, tgt, mask = run(ctx, group, 64, colours)
    plain = run(ctx, group, 64)
    for k, s in enumerate(group):
        want = T.get_patch_pair(s["patch"], s["back"], s["rec"], 64, colour=colours[k])
        d = np.abs(src[k].astype(np.float64) - want[0]) / 2
        print("%-28s colour: max |d| of the 0 .. 1 values = %.3g" % (s["name"], d.max()))
        assert d.max() <= 1e-5, s["name"]
        assert np.array_equal(tgt[k], plain[1][k]) and np.array_equal(mask[k], plain[2][k])      # the stage touches the image only
        assert np.abs(src[k] - plain[0][k]).max() > 1e-3                                        # and does act on it


def identity_sample(level=128):
    """A 128 x 128 constant grey patch (every xyz level set, so the mask is full) whose draws make every later stage the identity:
    the window is the patch, no rectangle, sigma 0, odd batch, angle 0, imsize 128 -- src is the colour stage's output times 2 - 1."""
    patch = np.full((128, 128, 6), level, np.uint8)
    back = np.full((300, 300, 3), 40, np.uint8)
    rec = {"v_ref": 50, "u_ref": 60, "v1": 50, "v2": 178, "u1": 60, "u2": 188, "side": 128, "shift_v": 0, "shift_u": 0,
           "rect": [[0, 0, 0, 0]] * 3, "even": 0, "sigma_edge": 0.0, "sigma_blur": 0.0, "sigma_ran": 0.0, "rot": [1, 0, 0, 0, 1, 0]}
    return {"patch": patch, "back": back, "rec": rec}


def noise_colour(seed, sample=0):
    return {"order": list(range(8)), "add": [0, 0, 0], "contrast": 1.0, "mul": [1, 1, 1], "blur_sigma": 0.0, "noise_scale": 10.0,
            "contrast2": [1, 1, 1], "sample": sample, "seed": seed}


def test_colour_stage_noise_statistics_and_keys(ctx):
    s = identity_sample()
    base = (np.float32(128) / np.float32(255) * np.float32(255)) / np.float32(255)
    a = run(ctx, [s, s], 128, [noise_colour(1234, 0), noise_colour(1234, 1)])[0]
    again = run(ctx, [s], 128, [noise_colour(1234, 0)])[0]
    other = run(ctx, [s], 128, [noise_colour(99, 0)])[0]
    assert np.array_equal(a[0], again[0])                       # the same seed and sample repeat bit for bit
    assert not np.array_equal(a[0], other[0]) and not np.array_equal(a[0], a[1])      # another seed, another sample: other noise
    v = (a[0].astype(np.float64) + 1) / 2                       # the 0 .. 1 patch after the stage, 128 * 128 values per channel
    for ch in range(3):
        mean, std = v[..., ch].mean() - float(base), v[..., ch].std()
        print("channel %d: mean shift %.3g (bound %.3g), std %.5g (10 / 255 = %.5g)" % (ch, mean, 0.5 / 255, std, 10 / 255))
        assert abs(mean) < 0.5 / 255 and abs(std / (10 / 255) - 1) < 0.05
    assert abs(np.corrcoef(v[..., 0].ravel(), v[..., 1].ravel())[0, 1]) < 0.05      # channels carry their own noise


def test_bad_samples_set_their_status_and_leave_the_others_alone(ctx, samples):
    """Host-side checks before any launch: a patch of 129 rows, a background smaller than the patch plus 20 after the enlargement
    rule, a draw that is not finite -- each marks its sample, whose outputs are 0; the good samples equal their solo results."""
    from pix2pose_amd import _lib
    good = [s for s in samples if s["imsize"] == 64][:2]
    tall = dict(good[0], patch=np.zeros((129, 40, 6), np.uint8))
    small = {"patch": np.full((12, 12, 6), 9, np.uint8), "back": np.zeros((20, 20, 3), np.uint8), "rec": good[0]["rec"]}
    nan = dict(good[1], rec=dict(good[1]["rec"], sigma_blur=float("nan")))
    group = [good[0], tall, small, good[1], nan]
    src, tgt, mask, status = run(ctx, group, 64, return_status=True)
    assert status.tolist() == [_lib.TRAIN_OK, _lib.TRAIN_BAD_PATCH, _lib.TRAIN_BAD_BACKGROUND, _lib.TRAIN_OK, _lib.TRAIN_BAD_DRAW]
    for k in (1, 2, 4):
        assert not src[k].any() and not tgt[k].any() and not mask[k].any()
    for k, s in ((0, good[0]), (3, good[1])):
        alone = run(ctx, [s], 64)
        assert np.array_equal(src[k], alone[0][0]) and np.array_equal(tgt[k], alone[1][0]) and np.array_equal(mask[k], alone[2][0])
    with pytest.raises(ValueError, match="left out"):
        run(ctx, group, 64)
    with pytest.raises(_lib.P2PError):
        run(ctx, good, 64, generation=0)
