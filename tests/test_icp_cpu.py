"""The ICP restatement (tests/icp_ref.py) against sources that do not share its derivation: a brute-force float32 scan for the
nearest neighbour (ties counted), sorting for the lower medians, an explicit Rz Ry Rx product for getTransformMat, numpy's lstsq for
the solve (a rank-deficient planar case included), cvRound's half-even on the pyramid constants, and a known answer: a closed
surface with analytic normals moved by 5 mm / 2 degrees is recovered, with and without 20 % outliers.

Bars of the known answer, measured from the restatement (seed 0) and recorded with about 3x headroom: without outliers 0.0063 deg /
0.0014 mm measured, bar 0.02 deg / 0.005 mm; with 20 % outliers 0.084 deg / 0.0104 mm measured, bar 0.25 deg / 0.03 mm."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ref as I  # noqa: E402


def ellipsoid(n, rs, axes=(0.05, 0.035, 0.025)):
    """n points of an ellipsoid surface (metres) with its analytic outward normals, float32 [n, 6]."""
    u = rs.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    a = np.asarray(axes)
    p = u * a
    nrm = p / a ** 2
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return np.hstack([p, nrm]).astype(np.float32)


def axis_angle(axis, deg):
    ax = np.asarray(axis, float)
    ax /= np.linalg.norm(ax)
    th = np.radians(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def moved(pc, R, t):
    return np.hstack([pc[:, :3] @ R.T + t, pc[:, 3:] @ R.T]).astype(np.float32)


def test_nearest_matches_brute_force_with_ties():
    rs = np.random.RandomState(3)
    # a lattice (many exact float32 ties at the cell midpoints), duplicated rows, and random points
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 0.25
    Q = np.concatenate([g, g[:17], rs.uniform(0, 1.5, (300, 3)).astype(np.float32)])
    Q = np.hstack([Q, np.zeros_like(Q)])
    M = np.concatenate([g + 0.125, g[:40] + np.float32(0.125) * np.array([1, 0, 0], np.float32), g[:30],
                        rs.uniform(-0.5, 2.0, (500, 3)).astype(np.float32)])
    jb, db = I.nearest_brute(M, Q)
    jk, dk = I.NearestQ(Q)(M)
    assert np.array_equal(db, dk)
    assert np.array_equal(jb, jk)
    # the ties are real: some rows have several equal minima, and the lowest row wins
    d = I.d2_f32(M[:, None, :], Q[None, :, :])
    nties = (d == d.min(axis=1, keepdims=True)).sum(axis=1)
    assert (nties > 1).sum() > 50
    assert all(jk[i] == np.nonzero(d[i] == d[i].min())[0][0] for i in np.nonzero(nties > 1)[0])


@pytest.mark.parametrize("n", [1, 2, 5, 6, 101, 1000])
def test_lower_median_and_rejection_threshold(n):
    rs = np.random.RandomState(n)
    v = (rs.rand(n) ** 3).astype(np.float32)
    assert I.lower_median(v) == np.sort(v)[(n - 1) // 2]
    keep = I.reject(v, 2.5)
    med = np.sort(v)[(n - 1) // 2]
    dev = np.sort(np.abs(v.astype(np.float64) - float(med)).astype(np.float32))[(n - 1) // 2]
    thr = np.float32(np.float32(2.5) * (np.float32(1.48257968) * dev)) + med
    assert np.array_equal(keep, v < thr)
    assert I.reject(v, 0.0).all() and I.reject(v, -1.0).all()


def test_even_count_takes_the_lower_median():
    d2 = np.array([1, 2, 3, 4, 100, 101], np.float32)      # lower median 3, upper 4
    med = I.lower_median(d2)
    assert med == 3
    # |d2 - 3| = 2 1 0 1 97 98 -> lower median 1: thr = 2.5 * 1.48257968 + 3 = 6.7064...
    keep = I.reject(d2, 2.5)
    assert keep.tolist() == [True, True, True, True, False, False]
    # the comparison is strict: med = 0 and lowermedian(dev) = 0 give thr = 0, and d2 = 0 is not kept
    d2 = np.array([0, 0, 0, 1, 1], np.float32)
    assert I.reject(d2, 2.5).tolist() == [False] * 5


def test_transform_mat_is_rz_ry_rx():
    rs = np.random.RandomState(1)
    for _ in range(20):
        x = rs.uniform(-3, 3, 6)

        def R(axis, a):
            c, s = np.cos(a), np.sin(a)
            m = np.eye(3)
            i, j = [(1, 2), (0, 2), (0, 1)][axis]
            m[i, i] = m[j, j] = c
            m[i, j], m[j, i] = (-s, s) if axis != 1 else (s, -s)
            return m
        want = R(2, x[2]) @ R(1, x[1]) @ R(0, x[0])
        X = I.transform_mat(x)
        np.testing.assert_allclose(X[:3, :3], want, atol=1e-15)
        np.testing.assert_array_equal(X[:3, 3], x[3:])
        np.testing.assert_array_equal(X[3], [0, 0, 0, 1])


def test_solve_matches_lstsq():
    rs = np.random.RandomState(2)
    P = ellipsoid(400, rs)
    Q = moved(ellipsoid(400, rs), axis_angle((1, 1, 0), 3), np.array([0.002, -0.001, 0.003]))
    A, b = I.point_to_plane_system(P, Q)
    x = I.solve_normal(A.T @ A, A.T @ b)
    want = np.linalg.lstsq(A, b, rcond=None)[0]
    np.testing.assert_allclose(x, want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()))


def test_solve_rank_deficient_planar_target_is_minimum_norm():
    rs = np.random.RandomState(4)
    p = np.hstack([rs.uniform(-1, 1, (200, 2)), np.zeros((200, 1))]).astype(np.float32)
    q = p + np.array([0.0, 0.0, 0.05], np.float32)
    n = np.tile(np.array([0, 0, 1], np.float32), (200, 1))
    A, b = I.point_to_plane_system(np.hstack([p, n]), np.hstack([q, n]))
    assert np.linalg.matrix_rank(A) == 3              # rotation about the normal and the in-plane translation are free
    x = I.solve_normal(A.T @ A, A.T @ b)
    want = np.linalg.lstsq(A, b, rcond=None)[0]          # lstsq: the minimum-norm solution
    np.testing.assert_allclose(x, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(x, [0, 0, 0, 0, 0, 0.05], atol=1e-12)


@pytest.mark.parametrize("n", [2047, 2049, 1023, 1025, 5, 7, 9, 13, 3])
def test_cv_round_half_even_on_pyramid_constants(n):
    for level in range(4):
        c = I.level_constants(n, 100, level, 100, 0.005)
        x = n / 2.0 ** level
        fl = np.floor(x)
        want = int(fl) if x - fl < 0.5 or (x - fl == 0.5 and fl % 2 == 0) else int(fl) + 1
        assert c["samples"] == want
        if want:
            y = n / float(want)
            fy = np.floor(y)
            assert c["step"] == (int(fy) if y - fy < 0.5 or (y - fy == 0.5 and fy % 2 == 0) else int(fy) + 1)
    assert I.level_constants(5, 9, 1, 100, 0.005)["samples"] == 2          # 2.5 -> 2
    assert I.level_constants(7, 9, 1, 100, 0.005)["samples"] == 4          # 3.5 -> 4
    assert I.level_constants(3, 9, 1, 100, 0.005)["step"] == 2             # samples 2 (1.5 -> 2), step 1.5 -> 2
    c = I.level_constants(3, 9, 1, 100, 0.005)
    assert (c["np"], c["nq"], c["max_it"]) == (1, 4, 50)


@pytest.mark.parametrize("outliers,rot_bar,t_bar_mm", [(0.0, 0.02, 0.005), (0.2, 0.25, 0.03)])
def test_known_motion_is_recovered(outliers, rot_bar, t_bar_mm):
    rs = np.random.RandomState(0)
    S = ellipsoid(3000, rs)
    T = ellipsoid(3000, rs)
    R, t = axis_angle((1, 2, 3), 2.0), np.array([3.0, -4.0, 0.0]) / 5.0 * 0.005        # 2 degrees, 5 mm
    T = moved(T, R, t)
    if outliers:
        k = int(outliers * len(T))
        idx = rs.choice(len(T), k, replace=False)
        T[idx, :3] += rs.uniform(-0.03, 0.03, size=(k, 3)).astype(np.float32)
    r = I.icp(S, T)
    assert r["status"] == 0
    assert I.rotation_error_deg(r["pose"][:3, :3], R) <= rot_bar
    assert 1000 * np.linalg.norm(r["pose"][:3, 3] - t) <= t_bar_mm
    # and the identity start is far from it: the ICP did the work
    assert I.rotation_error_deg(np.eye(3), R) > 1.9


def test_nonfinite_and_empty_levels():
    rs = np.random.RandomState(5)
    S = ellipsoid(50, rs)
    T = ellipsoid(50, rs)
    T[7, 1] = np.nan
    assert I.icp(S, T)["status"] == -3
    # n >> m: at level 1 the step comes from n, so Q can be empty there and that level runs no iteration
    S = ellipsoid(400, rs)
    r = I.icp(S, ellipsoid(1, rs), num_levels=2)
    assert r["iterations"][1] == 0 and r["pairs"][1] == 0
