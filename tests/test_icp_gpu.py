"""GPU tests of the point-to-plane ICP (p2p_icp_batch, csrc/icp.hip) against the numpy restatement (tests/icp_ref.py).

Correspondence, rejection and picky selection are exact: the pair counts (selInd) of every level and the iteration counts must be
equal.  The pose is compared within a bar, because the GPU reduces the normal equations and the residual in a fixed tree while the
restatement uses numpy's sums: 1e-10 after one iteration, 1e-9 (R entries, t in metres) with the default parameters (about 1e-15 was
measured).  fval_min per level is held to 1e-9 relative.  Batch invariance and the grid route against the brute-force route of the
development twin are bit for bit."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import icp_ref as I  # noqa: E402

pytestmark = pytest.mark.gpu

POSE_BAR = 1e-9
ONE_IT_BAR = 1e-10


@pytest.fixture(scope="module")
def ctx():
    from pix2pose_amd.runtime import Context
    c = Context(0, max_batch=8)
    yield c
    c.close()


def axis_angle(axis, deg):
    ax = np.asarray(axis, float)
    ax /= np.linalg.norm(ax)
    th = np.radians(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def cloud_pair(n, m, seed, outliers=0.1, deg=3.0, mm=8.0, z=0.7):
    """A source patch (the camera-facing half of an ellipsoid at depth z, metres) and a target of the same surface moved by deg / mm,
    sampled independently, with noise and a fraction of outliers.  float32 [n, 6], [m, 6]."""
    rs = np.random.RandomState(seed)
    a = np.array([0.05, 0.035, 0.025])

    def half(k):
        u = rs.normal(size=(k, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        u[:, 2] = -np.abs(u[:, 2])
        p = u * a
        nrm = p / a ** 2
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        return p + [0, 0, z], nrm
    ps, ns = half(n)
    pt, nt = half(m)
    R = axis_angle(rs.normal(size=3), deg)
    t = rs.normal(size=3)
    t = t / np.linalg.norm(t) * mm / 1000
    c = np.array([0, 0, z])
    pt = (pt - c) @ R.T + c + t + rs.normal(scale=0.0003, size=pt.shape)
    nt = nt @ R.T
    k = int(outliers * m)
    if k:
        idx = rs.choice(m, k, replace=False)
        pt[idx] += rs.uniform(-0.05, 0.05, size=(k, 3))
    return np.hstack([ps, ns]).astype(np.float32), np.hstack([pt, nt]).astype(np.float32)


def check(got, want, bar=POSE_BAR, levels=2):
    assert got["status"] == want["status"]
    assert got["iterations"][:levels] == want["iterations"][:levels]
    assert got["pairs"][:levels] == want["pairs"][:levels]
    for l in range(levels):
        assert abs(got["fval_min"][l] - want["fval_min"][l]) <= 1e-9 * abs(want["fval_min"][l]) + 1e-15, l
    err = np.abs(got["pose"] - want["pose"]).max()
    assert err <= bar, err
    assert got["scale"] == want["scale"]
    assert np.array_equal(got["mean_avg"], want["mean_avg"])
    return err


def run(ctx, pairs, **params):
    from pix2pose_amd import runtime
    return runtime.icp_batch(ctx, [{"status": 0}] * len(pairs), [p[0] for p in pairs], [p[1] for p in pairs], **params)


@pytest.mark.parametrize("n,m", [(500, 700), (3000, 2500), (20000, 20000)])
def test_one_iteration_pins_correspondence_rejection_and_picky(ctx, n, m):
    S, T = cloud_pair(n, m, n)
    got = run(ctx, [(S, T)], max_iterations=1, num_levels=1)[0]
    want = I.icp(S, T, max_iterations=1, num_levels=1)
    assert got["iterations"][0] == 1
    check(got, want, ONE_IT_BAR, levels=1)


@pytest.mark.parametrize("n,m", [(6, 6), (40, 55), (1000, 1000), (7001, 6003), (40000, 40000), (4000, 300), (300, 4000)],
                         ids=["6", "40x55", "1k", "7k", "40k", "n>>m", "n<<m"])
def test_default_parameters_match_the_restatement(ctx, n, m):
    S, T = cloud_pair(n, m, n + m)
    got = run(ctx, [(S, T)])[0]
    want = I.icp(S, T)
    check(got, want)
    if n >= 1000 and n == m:
        assert sum(want["iterations"]) > 2


@pytest.mark.parametrize("n,m,levels,seed", [(44, 52, 4, 500), (44, 60, 4, 500), (44, 100, 4, 501)])
def test_target_step_comes_from_the_source_count(ctx, n, m, levels, seed):
    """At level 1 rint(n / rint(n / 2)) = 2 for every n >= 2, so the target's step only depends on which count it comes from at deeper
    levels with few samples.  Here the coarsest level's step from n differs from rint(m / rint(m / 8)), and the restatement's pair
    counts differ between the two rules (checked on the host when the case was chosen)."""
    l = levels - 1
    c = I.level_constants(n, m, l, 100, 0.005)
    step_m = I.cv_round(m / float(I.cv_round(m / 2.0 ** l)))
    assert c["step"] != step_m and c["nq"] == m // c["step"]
    S, T = cloud_pair(n, m, seed, outliers=0)
    got = run(ctx, [(S, T)], num_levels=levels)[0]
    check(got, I.icp(S, T, num_levels=levels), levels=levels)


def test_planar_target_rejection_off_levels_ties_and_zero_normals(ctx):
    rs = np.random.RandomState(7)
    # planar target: the rotation about the normal and the in-plane translation are free (minimum-norm solve)
    p = np.hstack([rs.uniform(-0.05, 0.05, (800, 2)), np.full((800, 1), 0.6)])
    plane = np.hstack([p, np.tile([0.0, 0.0, -1.0], (800, 1))]).astype(np.float32)
    src = plane.copy()
    src[:, 2] += (0.004 + rs.normal(scale=1e-4, size=800)).astype(np.float32)     # (equal offsets: MAD 0, every pair rejected)
    cases = [(src, plane, {}), (src, plane, {"rejection_scale": 0.0}), (src, plane, {"rejection_scale": -2.0})]
    S, T = cloud_pair(1500, 1400, 11)
    for L in (1, 2, 3, 4):
        cases.append((S, T, {"num_levels": L}))
    # duplicated target rows (exact ties in the nearest neighbour and in the picky selection)
    Td = np.concatenate([T, T[::3], T[::5]])
    cases.append((S, Td, {}))
    # zero normals on both sides
    Sz, Tz = S.copy(), T.copy()
    Sz[::4, 3:] = 0
    Tz[::3, 3:] = 0
    cases.append((Sz, Tz, {}))
    cases.append((S, T, {"tolerance": 0.0, "max_iterations": 7}))
    for S_, T_, prm in cases:
        got = run(ctx, [(S_, T_)], **prm)[0]
        want = I.icp(S_, T_, **prm)
        check(got, want, levels=prm.get("num_levels", 2))
    # planar: the translation along the normal is recovered, the free directions stay at the minimum-norm 0
    got = run(ctx, [(src, plane)])[0]
    assert got["iterations"][0] > 0
    assert abs(got["pose"][2, 3] + 0.004) <= 2e-5
    assert np.abs(got["pose"][:2, 3]).max() <= 5e-4       # (measured 1.1e-4: the noise tilts the fit a little)


def test_break_below_six_pairs(ctx):
    S, T = cloud_pair(40, 5, 3, outliers=0)
    got = run(ctx, [(S, T)], num_levels=1)[0]
    want = I.icp(S, T, num_levels=1)
    assert want["iterations"][0] == 0 and 0 < want["pairs"][0] < 6
    check(got, want, levels=1)
    assert np.array_equal(got["pose"], np.eye(4))
    # every pair rejected (thr = 0 when more than half the distances are 0): selInd 0
    S = np.zeros((9, 6), np.float32)
    S[:, 3] = 1
    S[5:, 0] = np.arange(1, 5)
    got = run(ctx, [(S, S.copy())], num_levels=1)[0]
    want = I.icp(S, S.copy(), num_levels=1)
    assert want["pairs"][0] == 0
    check(got, want, levels=1)


def tie_case(seed=0):
    """A target grid on z = 0 with the origin as row 0, and a source symmetric under p -> -p (dyadic coordinates, so the float64 means
    are exactly 0 and the normalised coordinates stay exactly symmetric): several source rows have the same float32 d2 to target
    row 0, so the picky selection has ties to break."""
    rs = np.random.RandomState(seed)
    g = np.arange(-2, 3) / 4.0
    T = np.array([(0.0, 0.0, 0.0)] + [(x, y, 0.0) for x in g for y in g if (x, y) != (0.0, 0.0)])
    half = np.stack([rs.randint(-8, 9, 40) / 16.0, rs.randint(-8, 9, 40) / 16.0, rs.randint(1, 9, 40) / 32.0], 1)
    ties = np.array([[0.125, 0.0, 0.0625], [-0.125, 0.0, 0.0625]])
    S = np.concatenate([ties, half, -ties, -half])
    z = np.array([0.0, 0.0, 1.0])
    return (np.hstack([S, np.tile(z, (len(S), 1))]).astype(np.float32), np.hstack([T, np.tile(z, (len(T), 1))]).astype(np.float32))


def test_picky_ties_go_to_the_highest_source_row(ctx):
    S, T = tie_case()
    prm = dict(num_levels=1, max_iterations=1, rejection_scale=0.0)
    want = I.icp(S, T, **prm)
    assert np.array_equal(want["mean_avg"], np.zeros(3))
    s0, t0, _, _ = I.normalise(S, T)
    j, d2 = I.nearest_brute(s0, t0)
    on0 = d2[j == 0]
    assert (on0 == on0.min()).sum() >= 2                  # a real tie on target row 0
    got = run(ctx, [(S, T)], **prm)[0]
    check(got, want, ONE_IT_BAR, levels=1)
    # the other tie rule moves the pose far beyond the bar (0.019 measured), so the check above decides it
    i, jj = I.picky(j, d2, np.ones(len(j), bool))
    assert i[jj == 0][0] == np.nonzero((j == 0) & (d2 == on0.min()))[0].max()


def test_batch_invariance_256_jobs(ctx):
    pairs = [cloud_pair(200 + 37 * k, 150 + 53 * (k % 40), 1000 + k) for k in range(256)]
    allr = run(ctx, pairs)
    for k in (0, 1, 77, 128, 255):
        alone = run(ctx, [pairs[k]])[0]
        for key in ("pose", "fval_min", "iterations", "pairs", "scale", "mean_avg"):
            assert np.array_equal(np.asarray(alone[key]), np.asarray(allr[k][key])), (k, key)
    for k in (3, 200):
        check(allr[k], I.icp(*pairs[k]))


_BRUTE_SCRIPT = r"""
import sys, pickle
sys.path.insert(0, sys.argv[1])
from pix2pose_amd import runtime
a = pickle.load(open(sys.argv[2], "rb"))
ctx = runtime.Context(0, max_batch=8)
out = runtime.icp_batch(ctx, [{"status": 0}] * len(a["pairs"]), [p[0] for p in a["pairs"]], [p[1] for p in a["pairs"]])
pickle.dump(out, open(sys.argv[3], "wb"))
"""


def test_grid_route_equals_brute_force_route(ctx, tmp_path):
    from pix2pose_amd import build
    pairs = [cloud_pair(n, m, 90 + n) for n, m in ((6, 9), (900, 1300), (5000, 4000), (12000, 15000))]
    S, T = cloud_pair(1500, 1400, 11)
    pairs.append((S, np.concatenate([T, T[::3], T[::5]])))          # ties
    rs = np.random.RandomState(1)
    far = S.copy()
    far[:, :3] += rs.uniform(-1, 1, far[:, :3].shape).astype(np.float32) * 0.2   # queries far outside the grid
    pairs.append((far, T))
    grid = run(ctx, pairs)
    inp, outp = tmp_path / "in.pkl", tmp_path / "out.pkl"
    pickle.dump({"pairs": pairs}, open(inp, "wb"))
    env = dict(os.environ, **build.dev_switches(P2P_ICP_BRUTE=1))
    r = subprocess.run([sys.executable, "-c", _BRUTE_SCRIPT, ROOT, str(inp), str(outp)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    brute = pickle.load(open(outp, "rb"))
    for g, b in zip(grid, brute):
        for key in ("pose", "fval_min", "iterations", "pairs"):
            assert np.array_equal(np.asarray(g[key]), np.asarray(b[key])), key


def test_status_passthrough_nonfinite_and_argument_errors(ctx):
    from pix2pose_amd import _lib, runtime
    S, T = cloud_pair(300, 300, 5)
    Tn = T.copy()
    Tn[17, 2] = np.nan
    Si = S.copy()
    Si[3, 0] = np.inf
    out = runtime.icp_batch(ctx, [{"status": -1}, {"status": 0}, {"status": -2}, {"status": 0}, {"status": 0}],
                            [S, S, S, Si, S], [T, Tn, T, T, T])
    assert [o["status"] for o in out] == [-1, -3, -2, -3, 0]
    for o in out[:4]:
        assert np.array_equal(o["pose"], np.eye(4)) and o["iterations"] == [0] * 8
    assert np.array_equal(out[4]["pose"], runtime.icp_batch(ctx, [{"status": 0}], [S], [T])[0]["pose"])
    same = np.tile(S[:1], (20, 1))              # every point at the mean: no finite normalisation
    assert runtime.icp_batch(ctx, [{"status": 0}], [same], [same])[0]["status"] == -3 == I.icp(same, same)["status"]
    bad = [dict(num_levels=0), dict(num_levels=9), dict(max_iterations=0), dict(tolerance=float("nan")),
           dict(rejection_scale=float("inf"))]
    for prm in bad:
        with pytest.raises(_lib.P2PError):
            runtime.icp_batch(ctx, [{"status": 0}], [S], [T], **prm)
    with pytest.raises(_lib.P2PError):          # rint(1 / 2) = 0 samples at the top level
        runtime.icp_batch(ctx, [{"status": 0}], [S[:1]], [T])
    with pytest.raises(_lib.P2PError):          # no target point
        runtime.icp_batch(ctx, [{"status": 0}], [S], [T[:0]])
    runtime.icp_batch(ctx, [{"status": 0}], [S[:1]], [T], num_levels=1)
    L = _lib.lib()
    assert L.p2p_icp_batch(ctx.handle, None, -1, None, None, None, None) == -1        # P2P_ERR_INVALID_ARG
    assert L.p2p_icp_batch(ctx.handle, None, 0, None, None, None, None) == 0
    for which, typ in ((10, _lib.IcpParams), (11, _lib.IcpResult), (12, _lib.RefineResult)):
        assert L.p2p_abi_sizeof(which) == C.sizeof(typ)
    assert L.p2p_abi_sizeof(13) == -1
    assert L.p2p_abi_version() == 12
