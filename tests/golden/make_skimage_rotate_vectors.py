"""Writes tests/golden/skimage_rotate018.npz: outputs of the real skimage.transform.rotate(..., resize=True) of scikit-image 0.18.3,
stored as raw bits, for tests/test_xyz_rotate_cpu.py.  Run it under an interpreter that has scikit-image 0.18.3:

    python tests/golden/make_skimage_rotate_vectors.py

Per size (9 x 13, 17 x 24, 37 x 53) the inputs -- a float32 3-channel image of 8-bit levels over 255 and a float64 0 / 1 mask -- and per
angle 30 ... 330 the rotated image with cval 0, with cval 0.5 and the rotated mask.  The file holds data produced by scikit-image and
numpy's random generator, nothing else.
"""
import os
import warnings

import numpy as np
import skimage
from skimage.transform import rotate

SIZES = ((9, 13), (17, 24), (37, 53))
ANGLES = tuple(range(30, 360, 30))


def main():
    assert skimage.__version__ == "0.18.3", skimage.__version__
    warnings.filterwarnings("ignore")
    rng = np.random.RandomState(18)
    out = {"version": np.array(skimage.__version__)}
    for (h, w) in SIZES:
        img = (rng.randint(0, 256, (h, w, 3)) / 255).astype(np.float32)
        mask = np.zeros((h, w), np.float64)
        mask[h // 4:h - h // 5, w // 3:w - w // 4] = 1.0
        mask[rng.randint(0, h, 6), rng.randint(0, w, 6)] = 1.0
        key = "%dx%d" % (h, w)
        out[key + "_img"] = img.view(np.uint32)
        out[key + "_mask"] = mask.view(np.uint64)
        for a in ANGLES:
            r0 = rotate(img, a, resize=True, cval=0)
            r5 = rotate(img, a, resize=True, cval=0.5)
            rm = rotate(mask, a, resize=True)
            assert r0.dtype == np.float32 and r5.dtype == np.float32 and rm.dtype == np.float64
            out["%s_a%03d_c0" % (key, a)] = np.ascontiguousarray(r0).view(np.uint32)
            out["%s_a%03d_c5" % (key, a)] = np.ascontiguousarray(r5).view(np.uint32)
            out["%s_a%03d_m" % (key, a)] = np.ascontiguousarray(rm).view(np.uint64)
    fn = os.path.join(os.path.dirname(os.path.abspath(__file__)), "skimage_rotate018.npz")
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
