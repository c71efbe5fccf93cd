"""The REAL third-party libraries this image does carry -- scikit-image 0.18.3, scipy 1.7.1 and h5py 3.3.0 under
/opt/conda/bin/python3.9 (the default interpreter has none of them) -- executed from the CPU suite, so that every recorded run
re-derives the committed fixtures from the libraries themselves instead of trusting a file:

  * tests/golden/external_vectors.json ["resize"]            == tools/make_external_vectors.py run now
  * tests/test_convert_keras.py::test_read_hdf5_on_real_files under python3.9 (real h5py files; skipped under python3.10)

Skipped where that interpreter is missing."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY39 = "/opt/conda/bin/python3.9"


def _have(mod):
    if not os.path.exists(PY39):
        return False
    return subprocess.run([PY39, "-c", "import %s" % mod], capture_output=True).returncode == 0


def _run(args, timeout=600):
    env = dict(os.environ, PYTHONWARNINGS="ignore", PYTHONDONTWRITEBYTECODE="1")
    return subprocess.run([PY39] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.skipif(not _have("skimage"), reason="no /opt/conda/bin/python3.9 with scikit-image")
def test_committed_resize_vectors_are_what_the_real_skimage_produces(tmp_path):
    out = str(tmp_path / "ext.json")
    r = _run([os.path.join("tools", "make_external_vectors.py"), "--out", out])
    assert r.returncode == 0, r.stderr[-2000:]
    fresh = json.load(open(out))["resize"]
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "external_vectors.json")))["resize"]
    assert fresh["version"] == committed["version"] == "0.18.3"
    assert len(fresh["cases"]) == len(committed["cases"]) >= 20
    for a, b in zip(fresh["cases"], committed["cases"]):
        # float32 results: bit for bit on any machine (the matrix noise of the affine fit disappears in the cast to float32).  float64 / bool
        # results carry that noise (1e-14, BLAS-kernel dependent) in their bits, and at output sides that are multiples of 10 even in their
        # `> 0.9` decisions -- compared by value there.
        if b["out_dtype"] == "float32":
            for k in ("out_dtype", "crc", "u8_crc", "lt02_crc", "gt09_crc"):
                assert a[k] == b[k], (k, a["n_in"], a["n_out"], a["dtype"])
        elif a["n_out"] % 10:
            for k in ("out_dtype", "u8_crc", "lt02_crc", "gt09_crc"):
                assert a[k] == b[k], (k, a["n_in"], a["n_out"], a["dtype"])
        assert abs(a["sum"] - b["sum"]) < 1e-9 * max(1.0, abs(b["sum"]))


def test_bool_mask_filter_restatement_equals_scipy():
    """What csrc/pipeline.hip restates for generation 2 -- scipy.ndimage.gaussian_filter on a BOOL array: per axis
    t = x0 w0 + sum_{d = r .. 1} (x[-d] + x[+d]) w[d] in double, then a C cast to npy_bool -- against the scipy of THIS interpreter, for
    every crop side below 128 (the mask survives for some sides and vanishes entirely for others: the rounding of the weights' sum decides)."""
    import numpy as np
    from scipy import ndimage as ndi
    from pix2pose_amd import _lib
    import ctypes as C
    rs = np.random.RandomState(2)
    yy, xx = np.mgrid[:128, :128]
    m = (((yy - 60) ** 2 / 900 + (xx - 70) ** 2 / 1600) < 1) & (rs.rand(128, 128) > 0.02)
    L = _lib.lib()
    survived = set()
    for S in range(8, 128):
        sig = (128 / S - 1) / 2
        want = ndi.gaussian_filter(m, (sig, sig), cval=0, mode="constant")
        w = (C.c_double * 256)()
        r = L.p2p_aa_weights(S, w)
        wv = np.array(w[:r + 1])

        def axis_pass(a, axis):
            a = np.moveaxis(a.astype(np.float64), axis, 0)
            p = np.zeros((128 + 2 * r,) + a.shape[1:])
            p[r:r + 128] = a
            t = p[r:r + 128] * wv[0]
            for d in range(r, 0, -1):
                t = t + (p[r - d:r - d + 128] + p[r + d:r + d + 128]) * wv[d]
            return np.moveaxis(t.astype(np.uint8).astype(bool), 0, axis)
        got = axis_pass(axis_pass(m, 0), 1) if r > 0 else m
        # (the library's weights are built with libm's exp; numpy >= 1.19 evaluates exp with its own SIMD routine, 1 ulp apart on some
        # vectors -- where that moves the weights' sum across 1.0 the whole mask flips, so compare only where both builds of the weights agree)
        x = np.arange(-r, r + 1)
        phi = np.exp(-0.5 / (sig * sig) * x ** 2) if r > 0 else np.ones(1)
        if r > 0 and not np.array_equal(wv, (phi / phi.sum())[r:]):
            continue
        assert np.array_equal(got, want), S
        survived.add(bool(want.any()))
    assert survived == {True, False}


@pytest.mark.skipif(not _have("h5py"), reason="no /opt/conda/bin/python3.9 with h5py")
def test_hdf5_reader_on_real_h5py_files():
    """pix2pose_amd.convert_keras.read_hdf5 on files written by the real h5py 3.3.0: both Keras layouts, both backbones (row f-2)."""
    r = _run(["-m", "pytest", os.path.join("tests", "test_convert_keras.py"), "-q", "-p", "no:cacheprovider"])
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "skipped" not in tail.splitlines()[-1], tail
