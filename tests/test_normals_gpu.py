"""GPU tests of depth back-projection, normals and the ICP point sets (csrc/normals.hip) against the float64 restatement
(tests/normals_ref.py) and the reference's own lines (tests/golden/reference_normals.json): image sizes and cameras, NaN pixels and
holes wider than the fill, the bbox quirk and both gates at their edges, the 300 / 5000 mm bounds at their exact values, 256 jobs over
shared images, batch and region independence, the capacity retry and argument errors.

Tolerance (measured): points to 1e-6 relative per component (absolute below 1), counts / order / bbox / status exact, centroids to
1e-12 m.  The source points are compared with the restatement run on the depth the GPU rendered, so the test holds the normals and the
point sets, not the rasteriser (tests/test_depth_gpu.py does)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import depth_ref as D  # noqa: E402
import normals_ref as N  # noqa: E402
from golden.make_reference_normals_vectors import b64_f32, b64_u8  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pix2pose_amd.runtime import Context
    c = Context(0, max_batch=8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def meshes(ctx):
    from pix2pose_amd.runtime import Mesh
    box = D.box_mesh((-60.0, -45.0, -30.0), (60.0, 45.0, 30.0), 4)
    big = D.box_mesh((-400.0, -400.0, -20.0), (400.0, 400.0, 20.0), 2)       # covers the whole of a small image at 0.5 m
    return [box, D.l_mesh(6), big], [Mesh(ctx, *box), Mesh(ctx, *D.l_mesh(6)), Mesh(ctx, *big)]


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float((np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1.0)).max(initial=0))


def assert_points(got, want):
    e = rel_err(got, want)
    assert e <= 1e-6, e


def scene(H, W, K, seed, holes=True):
    """A sensor frame: a wavy wall with the box in front, zero and NaN pixels, and (holes) a hole wider than 2 L + 1 and a NaN block."""
    rs = np.random.RandomState(seed)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    d = (0.9 + 0.2 * np.sin(jj / 23.0) * np.cos(ii / 17.0) + 0.0003 * jj).astype(np.float32)
    obj = D.render_depth(*D.box_mesh((-60.0, -45.0, -30.0), (60.0, 45.0, 30.0), 4), K, D.rot(0, 30) @ D.rot(1, 20),
                         [0.0, 0.0, 600.0], H, W) if H >= 16 else np.zeros((H, W), np.float32)
    d = np.where(obj > 0, obj, d).astype(np.float32)
    d[rs.rand(H, W) < 0.05] = 0
    d[rs.rand(H, W) < 0.02] = np.nan
    if holes and H > 40 and W > 40:
        d[H // 5:H // 5 + 30, W // 6:W // 6 + 34] = 0
        d[H - 12:H - 4, 3:20] = np.nan
    return d


def job(K, t, mask, R=None, image=0, mesh=0):
    return {"mesh": mesh, "image": image, "camK": K, "R": np.eye(3) if R is None else R, "t": np.asarray(t, np.float64),
            "union_mask": mask}


def valid(d):
    d = np.nan_to_num(d)
    return (d > 0.2) & (d < 2.2)


def check_record(ctx, mlist, got, jb, depth, H, W, scene_pts=None):
    """One record of icp_inputs_batch against the restatement, on the depth the GPU renders at the record's t_init."""
    from pix2pose_amd import runtime
    K = np.asarray(jb["camK"], np.float64)
    sp = N.scene_points(depth, K) if scene_pts is None else scene_pts

    def render(t):
        np.testing.assert_allclose(t, got["t_init"], rtol=0, atol=1e-9)
        return runtime.render_depth_batch(ctx, mlist, [dict(jb, t=got["t_init"])], H, W)[0]

    want = N.icp_inputs(sp, jb["union_mask"], jb["t"], K, render)
    assert got["status"] == want["status"]
    assert got["bbox"] == want["bbox"]
    assert len(got["tgt"]) == len(want["tgt"]) and len(got["src"]) == len(want["src"])
    assert_points(got["tgt"], want["tgt"])
    assert_points(got["src"], want["src"])
    # (a NaN sensor pixel in the union makes the target centroid NaN, as np.mean does; NaN must then match NaN)
    for k, tol in (("centroid_tgt", 1e-12), ("centroid_src", 1e-12), ("t_init", 1e-9), ("t_adjusted", 1e-9)):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        assert np.nanmax(np.abs(got[k] - want[k]), initial=0) <= tol, k
    return max(rel_err(got["src"], want["src"]), rel_err(got["tgt"], want["tgt"]))


SIZES = [
    (480, 640, np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0, 0, 1]])),
    (540, 720, np.array([[1075.65, -2.5, 500.0], [0.0, 1073.9, 120.0], [0, 0, 1]])),        # integer cx, cy, skew
    (960, 1280, np.array([[2992.6, 4.0, 1000.4], [0.0, 2991.4, 300.6], [0, 0, 1]])),        # fractional either side of .5
    (37, 53, np.array([[60.0, 0.0, 40.7], [0.0, 61.0, 9.2], [0, 0, 1]])),
    (3, 40, np.array([[50.0, 0.0, 19.5], [0.0, 50.0, 1.5], [0, 0, 1]])),
]


@pytest.mark.parametrize("H,W,K", SIZES, ids=["640x480", "720x540", "1280x960", "53x37", "40x3"])
def test_depth_points_sizes_and_cameras(ctx, H, W, K):
    from pix2pose_amd import runtime
    imgs = [scene(H, W, K, 1), scene(H, W, K, 2, holes=False)]
    got = runtime.depth_points_batch(ctx, imgs, [K, K])
    for g, d in zip(got, imgs):
        assert_points(g, N.scene_points(d, K))
    alone = runtime.depth_points_batch(ctx, imgs[1:], [K])
    assert np.array_equal(alone[0], got[1], equal_nan=True)


def test_depth_points_all_zero_and_nan(ctx):
    from pix2pose_amd import runtime
    K = SIZES[3][2]
    z = np.zeros((37, 53), np.float32)
    n = np.full((37, 53), np.nan, np.float32)
    got = runtime.depth_points_batch(ctx, [z, n], [K, K])
    assert np.array_equal(got[0], np.zeros_like(got[0]))
    assert_points(got[1], N.scene_points(n, K))


def test_truncated_offsets_and_ignored_skew(ctx):
    from pix2pose_amd import runtime
    H, W = 6, 8
    d = np.ones((H, W), np.float32)
    K = np.array([[100.0, 0.0, 3.6], [0.0, 50.0, 2.4], [0, 0, 1]])
    Ks = K.copy()
    Ks[0, 1] = 9.0
    a, b = runtime.depth_points_batch(ctx, [d, d], [K, Ks])
    assert np.array_equal(a, b)
    assert a[0, 3, 0] == 0 and a[0, 4, 0] == 0 and a[0, 5, 0] == np.float32(0.01) and a[0, 2, 0] == np.float32(-0.01)
    assert a[2, 0, 1] == 0 and a[3, 0, 1] == 0 and a[4, 0, 1] == np.float32(0.02)


def test_icp_inputs_640_with_holes_and_nans(ctx, meshes):
    from pix2pose_amd import runtime
    mv, ml = meshes
    H, W, K = SIZES[0]
    d = scene(H, W, K, 7)
    R = D.rot(0, 30) @ D.rot(1, 20)
    m = np.zeros((H, W), bool)
    m[150:330, 220:430] = True
    jobs = [job(K, [0.0, 0.0, 605.0], m & valid(d), R), job(K, [4.0, -3.0, 250.0], m & valid(d), R, mesh=1),
            job(K, [0.0, 0.0, 600.0], np.zeros((H, W), bool), R)]
    got = runtime.icp_inputs_batch(ctx, ml, [d], jobs)
    sp = N.scene_points(d, K)
    errs = [check_record(ctx, ml, g, jb, d, H, W, sp) for g, jb in zip(got, jobs)]
    assert got[0]["status"] == 0 and len(got[0]["src"]) > 1000
    assert got[2]["status"] == -1 and len(got[2]["tgt"]) == 0 and np.isnan(got[2]["centroid_tgt"]).all()
    print("max rel err", max(errs))             # 0.0 on the MI355X: the same float32 bits


@pytest.mark.parametrize("H,W,K", SIZES[1:4], ids=["720x540", "1280x960", "53x37"])
def test_icp_inputs_sizes_and_cameras(ctx, meshes, H, W, K):
    from pix2pose_amd import runtime
    mv, ml = meshes
    d = scene(H, W, K, 11)
    R = D.rot(0, 30) @ D.rot(1, 20)
    jobs = [job(K, [0.0, 0.0, 610.0], valid(d), R), job(K, [0.0, 0.0, 620.0], valid(d), R, mesh=1)]
    got = runtime.icp_inputs_batch(ctx, ml, [d], jobs)
    sp = N.scene_points(d, K)
    for g, jb in zip(got, jobs):
        check_record(ctx, ml, g, jb, d, H, W, sp)


K48 = np.array([[80.0, 0.0, 31.63], [0.0, 82.5, 23.41], [0, 0, 1]])      # the 64 x 48 camera of the small-image tests


def _rect(H, W, r0, c0, r1, c1):
    m = np.zeros((H, W), bool)
    m[r0:r1, c0:c1] = True
    return m


def test_bbox_edges_and_border(ctx, meshes):
    """The big plate covers the whole 48 x 64 image, so init_mask = union_mask: bbox extents of exactly 4 and 5, bboxes on every
    image border, and the count gate with an extent of 5 in both axes."""
    from pix2pose_amd import runtime
    mv, ml = meshes
    H, W = 48, 64
    K = K48
    d = scene(H, W, K, 3)
    t = [0.0, 0.0, 500.0]
    sparse = np.zeros((H, W), bool)
    sparse[[10, 12, 15, 15], [20, 22, 25, 20]] = True
    masks = [_rect(H, W, 10, 10, 15, 40),            # rows 10..14: extent 4 -> gate
             _rect(H, W, 10, 10, 16, 40),            # extent 5 -> a 5-row crop
             _rect(H, W, 10, 10, 40, 15),            # 4 columns
             _rect(H, W, 10, 10, 40, 16),            # 5 columns
             _rect(H, W, 0, 0, 12, 20), _rect(H, W, 36, 44, 48, 64), _rect(H, W, 0, 0, H, W),
             sparse]
    jobs = [job(K, t, m, mesh=2) for m in masks]
    got = runtime.icp_inputs_batch(ctx, ml, [d], jobs)
    from pix2pose_amd import _lib
    assert [g["status"] for g in got] == [_lib.ICP_SMALL_BBOX, 0, _lib.ICP_SMALL_BBOX, 0, 0, 0, 0, _lib.ICP_FEW_POINTS]
    assert got[1]["bbox"] == [10, 10, 15, 39] and len(got[1]["src"]) == 5 * 29       # last row and column dropped
    assert got[5]["bbox"] == [36, 44, 47, 63]
    sp = N.scene_points(d, K)
    for g, jb in zip(got, jobs):
        check_record(ctx, ml, g, jb, d, H, W, sp)


def test_translation_bounds_at_their_exact_values(ctx, meshes):
    from pix2pose_amd import runtime
    mv, ml = meshes
    H, W = 48, 64
    K = K48
    d = scene(H, W, K, 4)
    m = _rect(H, W, 5, 5, 40, 60) & valid(d)
    zs = [300.0, np.nextafter(300.0, 0), np.nextafter(300.0, 1e9), 5000.0, np.nextafter(5000.0, 1e9), np.nextafter(5000.0, 0)]
    replaced = [False, True, False, False, True, False]
    got = runtime.icp_inputs_batch(ctx, ml, [d], [job(K, [1.0, 2.0, z], m) for z in zs])
    for g, z, rep in zip(got, zs, replaced):
        want = g["centroid_tgt"] * 1000.0 if rep else np.array([1.0, 2.0, z])
        assert np.array_equal(g["t_init"], want), (z, g["t_init"])


def test_256_jobs_over_shared_images(ctx, meshes):
    """The shape of tools/time_normals.py: 256 jobs over 4 frames (each frame named by 64 jobs, two cameras on one of them);
    a sample against the restatement, and bit-identity of a job alone and in the batch."""
    from pix2pose_amd import runtime
    mv, ml = meshes
    H, W, K = SIZES[0]
    K2 = K.copy()
    K2[0, 2] += 0.5
    imgs = [scene(H, W, K, 20 + i) for i in range(4)]
    rs = np.random.RandomState(0)
    jobs = []
    for k in range(256):
        i = k % 4
        r0, c0 = rs.randint(100, 300), rs.randint(150, 450)
        m = _rect(H, W, r0, c0, r0 + rs.randint(20, 160), c0 + rs.randint(20, 180)) & valid(imgs[i])
        R = D.rot(0, rs.uniform(-40, 40)) @ D.rot(1, rs.uniform(-40, 40))
        t = [rs.uniform(-60, 60), rs.uniform(-40, 40), rs.choice([rs.uniform(450, 800), 250.0, 6000.0])]
        jobs.append(job(K2 if (i == 3 and k % 8 == 7) else K, t, m, R, image=i, mesh=k % 2))
    got = runtime.icp_inputs_batch(ctx, ml, imgs, jobs)
    assert sum(g["status"] == 0 for g in got) > 100
    sp = {}
    for k in rs.choice(256, 6, replace=False).tolist() + [7, 15]:
        i, Kj = jobs[k]["image"], jobs[k]["camK"]
        key = (i, Kj is K2)
        if key not in sp:
            sp[key] = N.scene_points(imgs[i], Kj)
        check_record(ctx, ml, got[k], jobs[k], imgs[i], H, W, sp[key])
    for k in (0, 7, 100, 255):
        alone = runtime.icp_inputs_batch(ctx, ml, imgs, [jobs[k]])[0]
        for key in ("src", "tgt", "t_init", "t_adjusted", "centroid_src", "centroid_tgt"):
            assert np.array_equal(alone[key], got[k][key], equal_nan=True), (k, key)
        assert alone["bbox"] == got[k]["bbox"] and alone["status"] == got[k]["status"]


_REGION_SCRIPT = r"""
import sys, numpy as np, pickle
sys.path.insert(0, sys.argv[1])
from pix2pose_amd import runtime
a = pickle.load(open(sys.argv[2], "rb"))
ctx = runtime.Context(0, max_batch=8)
ml = [runtime.Mesh(ctx, v, t) for v, t in a["meshes"]]
out = runtime.icp_inputs_batch(ctx, ml, a["images"], a["jobs"])
pickle.dump(out, open(sys.argv[3], "wb"))
"""


def test_restricted_region_equals_whole_frame(ctx, meshes, tmp_path):
    """Fill and Gaussian of a job run over its crop grown by 8 + 2 L; the development twin's P2P_NORMALS_WHOLE=1 runs them over the
    whole frame.  The two give the same bits, on crops near the border and in the middle, with holes wider than the fill."""
    import pickle
    from pix2pose_amd import build, runtime
    mv, ml = meshes
    H, W, K = SIZES[0]
    imgs = [scene(H, W, K, 30)]
    R = D.rot(0, 30) @ D.rot(1, 20)
    d = imgs[0]
    jobs = [job(K, [0.0, 0.0, 600.0], valid(d), R), job(K, [0.0, 0.0, 600.0], _rect(H, W, 180, 250, 300, 400) & valid(d), R, mesh=1),
            job(K, [0.0, 0.0, 400.0], _rect(H, W, 0, 0, H, W), mesh=2), job(K, [0.0, 0.0, 400.0], _rect(H, W, 440, 600, H, W), mesh=2)]
    got = runtime.icp_inputs_batch(ctx, ml, imgs, jobs)
    assert all(g["status"] == 0 for g in got)
    inp, outp = tmp_path / "in.pkl", tmp_path / "out.pkl"
    pickle.dump({"meshes": mv, "images": imgs, "jobs": jobs}, open(inp, "wb"))
    env = dict(os.environ, **build.dev_switches(P2P_NORMALS_WHOLE=1))
    r = subprocess.run([sys.executable, "-c", _REGION_SCRIPT, ROOT, str(inp), str(outp)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    whole = pickle.load(open(outp, "rb"))
    for a, b in zip(got, whole):
        for key in ("src", "tgt", "t_adjusted", "centroid_src"):
            assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_capacity_retry(ctx, meshes):
    from pix2pose_amd import _lib, runtime
    mv, ml = meshes
    H, W = 48, 64
    K = K48
    d = scene(H, W, K, 5)
    jobs = [job(K, [0.0, 0.0, 500.0], _rect(H, W, 5, 5, 40, 50), mesh=2), job(K, [0.0, 0.0, 500.0], _rect(H, W, 20, 20, 30, 30), mesh=2)]
    want = runtime.icp_inputs_batch(ctx, ml, [d], jobs)
    keep = []
    arr = runtime._depth_jobs(jobs, keep)
    mh = (C.c_void_p * 3)(*[m.handle.value for m in ml])
    dp = (C.c_void_p * 1)(d.ctypes.data)
    res = (_lib.IcpInput * 2)()
    L = _lib.lib()
    n_src = sum(len(w["src"]) for w in want)
    n_tgt = sum(len(w["tgt"]) for w in want)
    src = np.zeros((n_src, 6), np.float32)
    tgt = np.zeros((n_tgt, 6), np.float32)
    rc = L.p2p_icp_inputs_batch(ctx.handle, mh, 3, dp, 1, arr, 2, H, W, res, src.ctypes.data, n_src - 1, tgt.ctypes.data, n_tgt)
    assert rc == _lib.ERR_CAPACITY
    assert [r.n_src for r in res] == [len(w["src"]) for w in want] and [r.n_tgt for r in res] == [len(w["tgt"]) for w in want]
    assert not src.any() and not tgt.any()
    rc = L.p2p_icp_inputs_batch(ctx.handle, mh, 3, dp, 1, arr, 2, H, W, res, None, 0, tgt.ctypes.data, n_tgt - 1)
    assert rc == _lib.ERR_CAPACITY
    rc = L.p2p_icp_inputs_batch(ctx.handle, mh, 3, dp, 1, arr, 2, H, W, res, None, 0, None, 0)      # records only
    assert rc == 0 and [r.n_src for r in res] == [len(w["src"]) for w in want]
    rc = L.p2p_icp_inputs_batch(ctx.handle, mh, 3, dp, 1, arr, 2, H, W, res, src.ctypes.data, n_src, tgt.ctypes.data, n_tgt)
    assert rc == 0
    assert np.array_equal(src, np.concatenate([w["src"] for w in want]), equal_nan=True)
    assert np.array_equal(tgt, np.concatenate([w["tgt"] for w in want]), equal_nan=True)


def test_argument_errors(ctx, meshes):
    from pix2pose_amd import _lib, runtime
    mv, ml = meshes
    K = K48
    for shape in ((2, 40), (40, 2), (2, 2)):
        with pytest.raises(_lib.P2PError, match="status -1"):
            runtime.depth_points_batch(ctx, [np.ones(shape, np.float32)], [K])
        with pytest.raises(_lib.P2PError, match="status -1"):
            runtime.icp_inputs_batch(ctx, ml, [np.ones(shape, np.float32)], [job(K, [0, 0, 500.0], np.ones(shape, bool))])
    d = np.ones((20, 30), np.float32)
    for bad in (np.array([[0.0, 0, 10], [0, 80, 10], [0, 0, 1]]), np.array([[80.0, 0, np.nan], [0, 80, 10], [0, 0, 1]]),
                np.array([[80.0, 0, 10], [0, 80, 1e5], [0, 0, 1]])):
        with pytest.raises(_lib.P2PError, match="status -1"):
            runtime.depth_points_batch(ctx, [d], [bad])
        with pytest.raises(_lib.P2PError, match="status -1"):
            runtime.icp_inputs_batch(ctx, ml, [d], [job(bad, [0, 0, 500.0], np.ones((20, 30), bool))])
    with pytest.raises(_lib.P2PError, match="status -1"):
        runtime.icp_inputs_batch(ctx, ml, [d], [dict(job(K, [0, 0, 500.0], np.ones((20, 30), bool)), image=1)])
    with pytest.raises(_lib.P2PError, match="status -1"):
        runtime.icp_inputs_batch(ctx, ml, [d], [job(K, [0, 0, 500.0], np.ones((20, 30), bool), mesh=3)])
    with pytest.raises(ValueError):
        runtime.icp_inputs_batch(ctx, ml, [d], [job(K, [0, 0, 500.0], None)])
    L = _lib.lib()
    assert L.p2p_depth_points_batch(ctx.handle, None, 1, None, 20, 30, None) == -1
    assert L.p2p_depth_points_batch(ctx.handle, None, 0, None, 20, 30, None) == 0
    assert L.p2p_abi_sizeof(9) == C.sizeof(_lib.IcpInput)


def test_golden_end_to_end(ctx):
    """tests/golden/reference_normals.json (the reference's getXYZ, get_normal and icp_refinement) through the runtime."""
    from pix2pose_amd import runtime
    G = json.load(open(os.path.join(HERE, "golden", "reference_normals.json")))
    H, W, K = G["H"], G["W"], np.array(G["K"])
    images = [b64_f32(s, (H, W)) for s in G["images"]]
    for d, s in zip(runtime.depth_points_batch(ctx, images, [K] * len(images)), G["scene_points"]):
        assert_points(d, b64_f32(s, (H, W, 6)))
    mesh = runtime.Mesh(ctx, np.array(G["mesh_verts"]), np.array(G["mesh_tris"]))
    jobs = [job(K, j["t"], b64_u8(j["union_mask"], (H, W)), np.array(G["R"]), image=j["image"]) for j in G["jobs"]]
    got = runtime.icp_inputs_batch(ctx, [mesh], images, jobs)
    for g, j in zip(got, G["jobs"]):
        assert (g["status"] != 0) == (j["status"] == -1), j["why"]
        assert g["bbox"] == j["bbox"] and len(g["tgt"]) == j["n_tgt"]
        assert_points(g["tgt"], b64_f32(G["scene_points"][j["image"]], (H, W, 6))[b64_u8(j["union_mask"], (H, W)) != 0])
        np.testing.assert_allclose(g["t_init"], j["t_init"], rtol=0, atol=2e-4)
        if j["status"] == 0:
            assert len(g["src"]) == j["n_src"]
            assert_points(g["src"], b64_f32(j["src"], (j["n_src"], 6)))
            np.testing.assert_allclose(g["t_adjusted"], j["t_adjusted"], rtol=0, atol=2e-4)
