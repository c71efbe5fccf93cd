"""Writes tests/golden/reference_train_batch.npz (inputs, draws), reference_train_batch_out<i>.npz (the outputs, in parts that each
stay below the size of the largest fixture the tree held before) and reference_train_generator.npz: outputs of the reference's own
pix2pose_util/data_io.py (get_patch_pair and generator()) under the real scikit-image 0.18.3, for tests/test_train_batch_cpu.py and
tests/test_train_batch_gpu.py.  Run it under an interpreter that has scikit-image 0.18.3, with the reference checkout's root as
argument:

    python tests/golden/make_reference_train_batch_vectors.py <reference root>

The reference's module is imported at run time; nothing of its text is copied.  Only what is missing is stood in: an `imgaug` module
whose augment_image returns its argument (the colour stage off), np.float (removed from numpy), and skimage.io.imread, which here
returns the synthetic backgrounds by file name.  random.random / random.gauss are wrapped to record the draws, and a profile hook reads
the integers get_patch_pair derived from them out of its frame when it returns.

Per case the seed is advanced until the case's condition holds (a clipped window, a negative rectangle start, ...) and until the one
value-dependent threshold has a margin: no window pixel with |radius - 0.3| < 1e-4.  (The other one, sum(xyz) > 0, is a sum of 8-bit
levels over 255: 0 or at least 1 / 255.)  Outputs are stored as int64 round(x * 2**36): 7e-12, two orders under the tests' 1e-9.
"""
import importlib.util
import os
import random
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SCALE = 2.0 ** 36
LIMIT = 520000
DRAWS = []
LOCALS = {}
BACKS = {}
REAL = []
KEEP = ("v_ref", "u_ref", "v1", "v2", "u1", "u2", "shift_v_min", "shift_u_min", "shift_v_max", "shift_u_max", "h_aug", "w_aug", "d_pos_v",
        "d_pos_u", "r_angle", "h")


def stand_ins():
    class Anything:
        def __init__(self, *a, **k):
            pass

        def augment_image(self, x):
            return x
    aug = types.ModuleType("imgaug.augmenters")
    aug.__getattr__ = lambda name: Anything
    pkg = types.ModuleType("imgaug")
    pkg.augmenters = aug
    sys.modules["imgaug"], sys.modules["imgaug.augmenters"] = pkg, aug
    if not hasattr(np, "float"):
        np.float = float
    import skimage.io
    skimage.io.imread = lambda fn: BACKS[os.path.basename(fn)]
    real_random, real_gauss = random.random, random.gauss
    REAL.append(real_random)

    def rec_random():
        DRAWS.append(real_random())
        return DRAWS[-1]

    def rec_gauss(mu, sigma):
        DRAWS.append(real_gauss(mu, sigma))
        return DRAWS[-1]
    random.random, random.gauss = rec_random, rec_gauss


def hook(frame, event, arg):
    if event == "return" and frame.f_code.co_name == "get_patch_pair":
        loc = frame.f_locals
        LOCALS.clear()
        LOCALS.update({k: float(loc[k]) if k in ("r_angle", "h") else int(loc[k]) for k in KEEP})
        LOCALS["side"] = int(loc["base_image"].shape[0])
        LOCALS["frame"] = tuple(int(v) for v in loc["back_img"].shape[:2])
        LOCALS["margin"] = float(np.abs(loc["radius"] - 0.3).min()) if "radius" in loc else np.inf


def patch(h, w, c, k):
    """A smooth synthetic train_xyz patch: an ellipse of xyz colours (0 outside), a textured rgb half, optionally a visibility channel."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    inside = ((y - h / 2 + 0.5) / (0.42 * h)) ** 2 + ((x - w / 2 + 0.5) / (0.40 * w)) ** 2 < 1
    p = np.zeros((h, w, c), np.uint8)
    for ch in range(3):
        p[..., ch] = np.clip(128 + 90 * np.sin(0.21 * (ch + 1) * y + 0.13 * x + k) * np.cos(0.09 * x - 0.05 * (ch + 2) * y), 0, 255)
    xyz = np.dstack([40 + 170 * x / max(1, w - 1), 30 + 190 * y / max(1, h - 1), 128 + 100 * np.sin(0.08 * (x + y) + k)])
    p[..., 3:6] = np.where(inside[..., None], np.clip(xyz, 1, 255), 0)
    p[~inside, :3] = 128
    if c == 7:
        p[..., 6] = inside * 255
    return p


def background(H, W, grey, k):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    # smooth, and periodic in 32 pixels along both axes so that the compressed fixture holds little more than one tile
    t = 2 * np.pi / 32
    b = np.dstack([128 + 100 * np.sin(t * (ch + 1) * x + 0.5 * k) * np.cos(t * y * (1 + ch % 2) - k) for ch in range(3)])
    b = np.clip(b, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(b[..., 0]) if grey else b


def d(i):
    return DRAWS[i]


def negative_start(dr, ph=128, Hb=256):
    """Cheap screen on the raw draws alone (the run itself confirms): the first rectangle's row start is negative."""
    v_ref = int(dr[1] * (Hb - ph - 20) + 10)
    height = ph * (1 + (dr[6] * 0.6 - 0.3))
    return int(int(v_ref + ph / 2) + (dr[9] - 0.5) * height) < 0


# name, patch (h, w, c), background (H, W), grey, batch_count, imsize, condition on LOCALS (and DRAWS), screen on the first 13 draws
CASES = [
    ("odd_nonsquare_37x61", (37, 61, 6), (150, 190), False, 1, 64, lambda L: True, None),
    ("even_128x90_7ch", (128, 90, 7), (260, 200), False, 0, 128, lambda L: True, None),
    ("grey_background", (48, 40, 6), (150, 170), True, 2, 64, lambda L: True, None),
    ("enlarged_one_axis", (60, 50, 6), (100, 180), False, 4, 64, lambda L: L["frame"] == (120, 180), None),
    ("clipped_top_left", (50, 50, 6), (110, 110), False, 6, 64, lambda L: L["shift_v_min"] > 0 and L["shift_u_min"] > 0, None),
    ("clipped_bottom_right", (50, 50, 6), (110, 110), False, 8, 64, lambda L: L["shift_v_max"] < 0 and L["shift_u_max"] < 0, None),
    ("negative_rectangle_start", (128, 128, 6), (256, 256), False, 3, 64,
     lambda L: L["h_aug"] > 0 and L["w_aug"] > 0 and L["d_pos_v"] < 0, negative_start),
    ("second_rectangle_h_aug_0", (24, 20, 6), (90, 100), False, 10, 128, lambda L: int(d(14) * 0.5 * L["h"]) == 0, None),
    ("sigmas_radius_0", (40, 44, 6), (150, 170), False, 12, 64, lambda L: d(11) * 2 < 0.125 and d(12) * 2 < 0.125, lambda dr: dr[11] * 2 < 0.125 and dr[12] * 2 < 0.125),
    ("sigmas_near_2", (40, 44, 6), (150, 170), False, 5, 64, lambda L: d(11) * 2 > 1.8 and d(12) * 2 > 1.8, lambda dr: dr[11] * 2 > 1.8 and dr[12] * 2 > 1.8),
]


def quant(a):
    return np.round(np.asarray(a, np.float64) * SCALE).astype(np.int64)


def main():
    import skimage
    assert skimage.__version__ == "0.18.3", skimage.__version__
    warnings.filterwarnings("ignore")
    stand_ins()
    spec = importlib.util.spec_from_file_location("reference_data_io", os.path.join(sys.argv[1], "pix2pose_util", "data_io.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    sys.setprofile(hook)
    out = {"version": np.array(skimage.__version__), "scale": np.array(SCALE), "names": np.array([c[0] for c in CASES])}
    seed = 1000
    with tempfile.TemporaryDirectory() as tmp:
        data_dir, back_dir = os.path.join(tmp, "data"), os.path.join(tmp, "back")
        os.makedirs(data_dir)
        os.makedirs(back_dir)
        for k, (name, pshape, bshape, grey, batch_count, imsize, cond, screen) in enumerate(CASES):
            p, b = patch(*pshape, k), background(*bshape, grey, k)
            np.save(os.path.join(data_dir, "%d.npy" % k), p)
            BACKS.clear()
            BACKS.update({"a": b, "b": b})
            gen = ref.data_generator(data_dir, back_dir, batch_size=1, imsize=imsize)
            gen.datafiles, gen.backfiles, gen.n_background = ["%d.npy" % k], ["a", "b"], 2
            while True:
                seed += 1
                random.seed(seed)
                if screen is not None and not screen([REAL[0]() for _ in range(13)]):
                    continue
                random.seed(seed)
                del DRAWS[:]
                s, t, m = gen.get_patch_pair(0, batch_count)
                if cond(LOCALS) and LOCALS["margin"] >= 1e-4:
                    break
            assert s.dtype == np.float64 and t.dtype == np.float64 and m.dtype == np.float64
            sums = p[..., 3:6].astype(np.float32).sum(axis=2) / 255
            assert not ((sums != 0) & (np.abs(sums) < 1e-6)).any()
            ints = dict(LOCALS)
            out.update({"patch_%d" % k: p, "back_%d" % k: b, "seed_%d" % k: np.array(seed), "batch_count_%d" % k: np.array(batch_count),
                        "imsize_%d" % k: np.array(imsize), "draws_%d" % k: np.array(DRAWS, np.float64).view(np.uint64),
                        "ints_%d" % k: np.array([ints[f] for f in KEEP[:10]] + [ints["side"], ints["frame"][0], ints["frame"][1]], np.int64),
                        "angle_%d" % k: np.array(ints["r_angle"]).view(np.uint64), "margin_%d" % k: np.array(ints["margin"]),
                        "src_%d" % k: quant(s), "tgt_%d" % k: quant(t), "mask_%d" % k: quant(m)})
            print(name, "seed", seed, "draws", len(DRAWS), "margin %.3g" % ints["margin"], ints)
    # inputs, draws and integers in reference_train_batch.npz; the outputs packed greedily into parts below LIMIT bytes each
    import io
    outputs = {k: out.pop(k) for k in list(out) if k.split("_")[0] in ("src", "tgt", "mask")}
    parts, sizes = [{}], [0]
    for k in range(len(CASES)):
        item = {key: outputs[key] for key in ("src_%d" % k, "tgt_%d" % k, "mask_%d" % k)}
        buf = io.BytesIO()
        np.savez_compressed(buf, **item)
        if sizes[-1] and sizes[-1] + buf.tell() > LIMIT:
            parts.append({})
            sizes.append(0)
        parts[-1].update(item)
        sizes[-1] += buf.tell()
    out["n_parts"] = np.array(len(parts))
    for fn, content in [("reference_train_batch.npz", out)] + [("reference_train_batch_out%d.npz" % i, p) for i, p in enumerate(parts)]:
        fn = os.path.join(HERE, fn)
        np.savez_compressed(fn, **content)
        print(fn, os.path.getsize(fn), "bytes")
        assert os.path.getsize(fn) < 590000

    # one generator() run: four views, three backgrounds, batch_size 3, two batches (batch_count 0 and 1) at imsize 64
    gout = {"version": np.array(skimage.__version__), "scale": np.array(SCALE)}
    shapes = [((44, 36, 6), 0), ((30, 52, 6), 1), ((64, 64, 7), 2), ((25, 25, 6), 3)]
    backs = [((120, 140), False, 4), ((140, 130), True, 5), ((100, 100), False, 6)]
    with tempfile.TemporaryDirectory() as tmp:
        data_dir, back_dir = os.path.join(tmp, "data"), os.path.join(tmp, "back")
        os.makedirs(data_dir)
        os.makedirs(back_dir)
        BACKS.clear()
        for k, (ps, kk) in enumerate(shapes):
            gout["patch_%d" % k] = patch(*ps, kk)
            np.save(os.path.join(data_dir, "view%d.npy" % k), gout["patch_%d" % k])
        for k, (bs, grey, kk) in enumerate(backs):
            gout["back_%d" % k] = BACKS["back%d.npy" % k] = background(*bs, grey, kk)
        gseed = 77
        while True:
            gseed += 1
            gen = ref.data_generator(data_dir, back_dir, batch_size=3, imsize=64)
            gen.datafiles = ["view%d.npy" % k for k in range(4)]
            gen.backfiles, gen.n_background = ["back%d.npy" % k for k in range(3)], 3
            random.seed(gseed)
            np.random.seed(gseed)
            margins = []
            it = gen.generator()
            real_hook = hook

            def hook2(frame, event, arg):
                real_hook(frame, event, arg)
                if event == "return" and frame.f_code.co_name == "get_patch_pair":
                    margins.append(LOCALS["margin"])
            sys.setprofile(hook2)
            batches = []
            for _ in range(2):
                bsrc, btgt, bdisc, bprob = next(it)
                batches.append((bsrc.copy(), btgt.copy(), bdisc.copy(), bprob.copy()))
            sys.setprofile(hook)
            if min(margins) >= 1e-4:
                break
        gout["seed"] = np.array(gseed)
        gout["datafiles"], gout["backfiles"] = np.array(gen.datafiles), np.array(gen.backfiles)
        for k, (bsrc, btgt, bdisc, bprob) in enumerate(batches):
            assert bsrc.shape == (3, 64, 64, 3) and bprob.shape == (3, 64, 64, 1) and bdisc.shape == (3,)
            gout.update({"src_%d" % k: quant(bsrc), "tgt_%d" % k: quant(btgt), "disc_%d" % k: bdisc, "prob_%d" % k: quant(bprob)})
    sys.setprofile(None)
    fn = os.path.join(HERE, "reference_train_generator.npz")
    np.savez_compressed(fn, **gout)
    print(fn, os.path.getsize(fn), "bytes", "seed", gseed)


if __name__ == "__main__":
    main()
