"""CPU tests of the float64 restatement of depth back-projection, normals and the ICP point sets (tests/normals_ref.py): it
reproduces the reference's own lines (tests/golden/reference_normals.json), its Gaussian and gradient are scipy's and numpy's, the
onion-peel depth does not reach the pixels that are consumed, and the int16 offsets and the ignored skew are pinned."""
import json
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_ref as D  # noqa: E402
import normals_ref as N  # noqa: E402
from golden.make_reference_normals_vectors import b64_f32, b64_u8  # noqa: E402

GOLD = json.load(open(os.path.join(HERE, "golden", "reference_normals.json")))
GH, GW = GOLD["H"], GOLD["W"]
GK = np.array(GOLD["K"])
GMESH = (np.array(GOLD["mesh_verts"]), np.array(GOLD["mesh_tris"]))
GIMAGES = [b64_f32(s, (GH, GW)) for s in GOLD["images"]]
GSCENE = [b64_f32(s, (GH, GW, 6)) for s in GOLD["scene_points"]]


def assert_points(got, want, rtol=1e-6):
    """float32 points to 1e-6 relative per component (absolute 1e-6 for components below 1, which normals and metre xyz are)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1.0)
    assert err.max(initial=0) <= rtol, err.max()
    return float(err.max(initial=0))


def test_scene_points_reproduce_the_reference():
    for d, want in zip(GIMAGES, GSCENE):
        assert_points(N.scene_points(d, GK), want)


@pytest.mark.parametrize("k", range(len(GOLD["jobs"])))
def test_icp_inputs_reproduce_the_reference(k):
    j = GOLD["jobs"][k]
    union = b64_u8(j["union_mask"], (GH, GW)) != 0
    scene = N.scene_points(GIMAGES[j["image"]], GK)
    got = N.icp_inputs(scene, union, j["t"], GK, lambda t: D.render_depth(*GMESH, GK, GOLD["R"], t, GH, GW))
    assert (got["status"] != 0) == (j["status"] == -1), j["why"]
    assert got["bbox"] == j["bbox"]
    assert len(got["tgt"]) == j["n_tgt"]
    assert_points(got["tgt"], GSCENE[j["image"]][union])
    np.testing.assert_allclose(got["t_init"], j["t_init"], rtol=0, atol=2e-4)          # mm; the reference's float32 means
    if j["status"] == -1:
        assert len(got["src"]) == 0
        return
    assert len(got["src"]) == j["n_src"]
    assert_points(got["src"], b64_f32(j["src"], (j["n_src"], 6)))
    np.testing.assert_allclose(got["t_adjusted"], j["t_adjusted"], rtol=0, atol=2e-4)


def test_golden_covers_both_gates_and_both_replacements():
    why = {j["why"]: j for j in GOLD["jobs"]}
    assert why["bbox gate (4 rows)"]["bbox"][2] - why["bbox gate (4 rows)"]["bbox"][0] == 3
    cg = why["count gate"]
    assert cg["bbox"][2] - cg["bbox"][0] >= 5 and cg["bbox"][3] - cg["bbox"][1] >= 5 and cg["status"] == -1
    for k in ("t < 300 replaced", "t > 5000 replaced"):
        assert why[k]["status"] == 0 and abs(why[k]["t_init"][2] - why[k]["t"][2]) > 100
    assert any(np.isnan(d).any() for d in GIMAGES)


@pytest.mark.parametrize("shape", [(48, 64), (3, 17), (17, 3), (3, 3), (37, 53), (5, 9)])
def test_gaussian_and_gradient_are_scipy_and_numpy(shape):
    f = np.random.RandomState(shape[0] * 100 + shape[1]).rand(*shape) * 2.0
    assert np.abs(N.gaussian(f) - ndimage.gaussian_filter(f, 2)).max() <= 1e-12
    g = np.gradient(f, 2, edge_order=2)
    assert np.array_equal(N.gradient(f, 0), g[0]) and np.array_equal(N.gradient(f, 1), g[1])


def test_gauss_weights_are_scipys():
    from scipy.ndimage._filters import _gaussian_kernel1d
    assert np.abs(np.array(N.gauss_weights()) - _gaussian_kernel1d(2, 0, 8)[8:]).max() <= 1e-16


def _holey(H, W, seed):
    rs = np.random.RandomState(seed)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    d = (0.8 + 0.3 * np.sin(jj / 7.0) * np.cos(ii / 5.0)).astype(np.float32)
    d[rs.rand(H, W) < 0.1] = 0
    d[rs.rand(H, W) < 0.03] = np.nan
    d[10:40, 5:38] = 0                          # wider than 2 L + 1: the fill does not reach its centre
    return d


def test_fill_depth_does_not_reach_consumed_pixels():
    d = _holey(50, 70, 3)
    K = np.array([[90.0, 0.0, 34.6], [0.0, 88.0, 24.2], [0, 0, 1]])
    on = np.nan_to_num(d) > 0
    a, b = N.scene_points(d, K), N.scene_points(d, K, layers=N.FILL_LAYERS + 5)
    assert np.array_equal(a[on], b[on])
    assert not np.array_equal(a[~on], b[~on])        # the fill does matter elsewhere, so this is not vacuous
    c = N.scene_points(d, K, layers=N.FILL_LAYERS - 3)
    assert not np.array_equal(a[on], c[on])           # and 10 is not more than needed here
    bbox = np.array([12, 30, 45, 66])
    m = on[bbox[0]:bbox[2], bbox[1]:bbox[3]]
    assert np.array_equal(N.points(d, K, bbox)[m], N.points(d, K, bbox, N.FILL_LAYERS + 5)[m])


def test_onion_peel_layers():
    d = np.zeros((9, 9), np.float32)
    d[4, 4] = 2.0
    d[0, 0] = 1.0
    f1 = N.inpaint(d, 1)
    assert f1[3, 3] == 2.0 and f1[1, 1] == 1.0 and f1[1, 0] == 1.0 and f1[2, 2] == 0 and f1[1, 2] == 0     # 8-neighbours only
    f2 = N.inpaint(d, 2)
    assert f2[2, 2] == 1.5          # its 5 x 5 window after layer 1: (0..1, 0..1) = 1 and (3..4, 3..4) = 2
    assert N.inpaint(np.zeros((5, 5), np.float32)).max() == 0


def test_int16_truncation_and_ignored_skew():
    H, W = 6, 8
    d = np.full((H, W), 1.0, np.float32)
    K = np.array([[100.0, 0.0, 3.6], [0.0, 50.0, 2.4], [0, 0, 1]])
    xyz = N.get_xyz(d, K)
    assert xyz[0, 3, 0] == 0.0 and xyz[0, 4, 0] == 0.0                # 3 - 3.6 = -0.6 -> 0 and 4 - 3.6 = 0.4 -> 0, not rounded
    assert xyz[0, 2, 0] == -1.0 / 100.0 and xyz[0, 5, 0] == 1.0 / 100.0
    assert xyz[2, 0, 1] == 0.0 and xyz[3, 0, 1] == 0.0 and xyz[4, 0, 1] == 1.0 / 50.0
    Ks = K.copy()
    Ks[0, 1] = 7.5
    d2 = _holey(20, 24, 1)
    assert np.array_equal(N.scene_points(d2, K), N.scene_points(d2, Ks), equal_nan=True)
    # the rasteriser does use the skew
    v, t = D.box_mesh((-20.0, -20.0, -20.0), (20.0, 20.0, 20.0), 2)
    Kr = np.array([[60.0, 0.0, 12.0], [0.0, 60.0, 10.0], [0, 0, 1]])
    Krs = Kr.copy()
    Krs[0, 1] = 15.0
    a = D.render_depth(v, t, Kr, np.eye(3), [0, 0, 400.0], 20, 24)
    b = D.render_depth(v, t, Krs, np.eye(3), [0, 0, 400.0], 20, 24)
    assert not np.array_equal(a > 0, b > 0)
