"""numpy restatement of the point-to-plane ICP of DESIGN.md section 8.2 (cv::ppf_match_3d::ICP::registerModelToScene as this library
defines it) and of the refinement around it (icp_refinement :86-94).  Precisions and rounding points are the ones DESIGN states:
float32 distances with the float32 nearest-neighbour rule, float64 transforms and solve, sequential float64 sums for the
normalisation.  The GPU agrees with it bit for bit up to the 6 x 6 solve and the fval sum (whose summation orders differ).

Nearest neighbours come from scipy's cKDTree as candidates; the float32 distance rule and the tie rule (lowest target row) are then
applied among every candidate that could tie, so the answer equals a brute-force float32 scan."""
import numpy as np
from scipy.spatial import cKDTree

F32 = np.float32
FVAL_INIT = 9999999999.0
NORMAL_EPS = 2.22e-16
EIG_REL = 1e-12
DEFAULTS = dict(max_iterations=100, tolerance=0.005, rejection_scale=2.5, num_levels=2)


def cv_round(v):
    """cvRound: round half to even."""
    return int(np.rint(v))


def level_constants(n, m, level, max_iterations, tolerance):
    """numSamples, step, |P|, |Q|, TolP, maxIt of pyramid level `level` (0 = finest) for n source and m target rows."""
    samples = cv_round(n / float(2 ** level))
    if samples == 0:        # the library refuses such a job (P2P_ERR_INVALID_ARG)
        return dict(samples=0, step=None, np=0, nq=0, tolp=None, max_it=None)
    step = cv_round(n / float(samples))
    return dict(samples=samples, step=step, np=n // step, nq=m // step,
                tolp=float(np.float32(tolerance)) * float((level + 1) ** 2), max_it=cv_round(max_iterations / float(level + 1)))


def seq_sum(x):
    """Left-to-right float64 sum (np.add.accumulate is sequential)."""
    x = np.asarray(x, np.float64)
    return np.add.accumulate(x, axis=0)[-1] if len(x) else np.zeros(x.shape[1:])


def normalise(S, T):
    """Step 1: returns S0, T0 (float32 [k, 6]), meanAvg (float64 [3]), scale (float64)."""
    n, m = len(S), len(T)
    mean_src = seq_sum(S[:, :3].astype(np.float64)) / n
    mean_dst = seq_sum(T[:, :3].astype(np.float64)) / m
    mean_avg = 0.5 * (mean_src + mean_dst)
    mf = mean_avg.astype(F32)
    sc = S[:, :3].astype(F32) - mf
    tc = T[:, :3].astype(F32) - mf

    def dist(a):
        a = a.astype(np.float64)
        return seq_sum(np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]))

    scale = float(n) / ((dist(sc) + dist(tc)) * 0.5)
    s0 = S.astype(F32).copy()
    t0 = T.astype(F32).copy()
    s0[:, :3] = sc * F32(scale)
    t0[:, :3] = tc * F32(scale)
    return s0, t0, mean_avg, scale


def transform(X, pc, normals=True):
    """transformPCPose: xyz = float32(R p + t) in float64, normal = float32(R n / |R n|), 0 where |R n| <= 2.22e-16."""
    X = np.asarray(X, np.float64)
    p = pc[:, :3].astype(np.float64)
    out = np.zeros((len(pc), 6 if normals else 3), F32)
    for r in range(3):
        out[:, r] = (((X[r, 0] * p[:, 0] + X[r, 1] * p[:, 1]) + X[r, 2] * p[:, 2]) + X[r, 3]).astype(F32)
    if normals:
        nv = pc[:, 3:6].astype(np.float64)
        n2 = np.stack([(X[r, 0] * nv[:, 0] + X[r, 1] * nv[:, 1]) + X[r, 2] * nv[:, 2] for r in range(3)], axis=1)
        nn = np.sqrt((n2[:, 0] * n2[:, 0] + n2[:, 1] * n2[:, 1]) + n2[:, 2] * n2[:, 2])
        ok = nn > NORMAL_EPS
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, 3:6] = np.where(ok[:, None], n2 / nn[:, None], 0.0).astype(F32)
    return out


def d2_f32(a, b):
    """float32 (dx dx + dy dy) + dz dz, dx = a.x - b.x in float32."""
    d = a[..., :3].astype(F32) - b[..., :3].astype(F32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest_brute(M, Q):
    """Brute-force float32 scan: least (d2, j) per row of M."""
    d = d2_f32(M[:, None, :], Q[None, :, :])
    j = np.argmin(d, axis=1)            # argmin returns the first (lowest j) of equal minima
    return j, d[np.arange(len(M)), j]


class NearestQ:
    """Exact float32 nearest neighbour in Q with ties to the lowest row (kd-tree candidates, float32 rule among them)."""

    def __init__(self, Q):
        self.Q = np.ascontiguousarray(Q[:, :3], F32)
        self.tree = cKDTree(self.Q.astype(np.float64))

    def __call__(self, M):
        Mx = np.ascontiguousarray(M[:, :3], F32)
        k = min(8, len(self.Q))
        dist, idx = self.tree.query(Mx.astype(np.float64), k=k)
        dist, idx = dist.reshape(len(Mx), k), idx.reshape(len(Mx), k)
        d2 = d2_f32(Mx[:, None, :], self.Q[idx])
        # among the k candidates: least (d2, j)
        best = np.full(len(Mx), np.inf, F32)
        bj = np.full(len(Mx), np.iinfo(np.int64).max, np.int64)
        for c in range(k):
            better = (d2[:, c] < best) | ((d2[:, c] == best) & (idx[:, c] < bj))
            best = np.where(better, d2[:, c], best)
            bj = np.where(better, idx[:, c], bj)
        # rows where a point beyond the k-th could still tie: every point within the (generous) float32 margin of the k-th's radius
        r2 = dist[:, 0].astype(np.float64) ** 2
        unsure = dist[:, -1].astype(np.float64) ** 2 <= r2 * (1 + 1e-5) + 1e-30
        if k == len(self.Q):
            unsure[:] = False
        for i in np.nonzero(unsure)[0]:
            cand = np.asarray(self.tree.query_ball_point(Mx[i].astype(np.float64), np.sqrt(r2[i] * (1 + 1e-5) + 1e-30)), np.int64)
            cand = np.union1d(cand, idx[i])
            dd = d2_f32(Mx[i][None, :], self.Q[cand])
            o = np.lexsort((cand, dd))[0]
            best[i], bj[i] = dd[o], cand[o]
        return bj, best


def lower_median(v):
    v = np.asarray(v)
    return np.partition(v, (len(v) - 1) // 2)[(len(v) - 1) // 2]


def reject(d2, rejection_scale):
    """Robust rejection (only when rejection_scale > 0): keep d2 < rho * 1.48257968 * lowermedian(|d2 - med|) + med (float32)."""
    if not rejection_scale > 0:
        return np.ones(len(d2), bool)
    med = F32(lower_median(d2))
    dev = np.abs(d2.astype(np.float64) - np.float64(med)).astype(F32)
    s = F32(1.48257968) * F32(lower_median(dev))
    thr = F32(F32(rejection_scale) * s) + med
    return d2 < thr


def picky(j, d2, keep):
    """Per target row the kept pair of least d2, ties to the highest i: (i, j) arrays in ascending j."""
    i = np.nonzero(keep)[0]
    jj, dd = j[i], d2[i]
    o = np.lexsort((-i, dd, jj))
    i, jj = i[o], jj[o]
    first = np.ones(len(jj), bool)
    first[1:] = jj[1:] != jj[:-1]
    return i[first], jj[first]


def jacobi6(a):
    """The kernel's cyclic Jacobi of a symmetric 6 x 6 (same loop, same operations): eigenvalues, eigenvectors (columns)."""
    a = [list(map(float, r)) for r in np.asarray(a, np.float64)]
    v = [[1.0 if r == c else 0.0 for c in range(6)] for r in range(6)]
    for _ in range(50):
        rotated = False
        for p in range(5):
            for q in range(p + 1, 6):
                apq = a[p][q]
                if abs(apq) <= 1e-18 * (abs(a[p][p]) + abs(a[q][q])):
                    a[p][q] = 0.0
                    a[q][p] = 0.0
                    continue
                rotated = True
                theta = (a[q][q] - a[p][p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + float(np.sqrt(theta * theta + 1.0)))
                c = 1.0 / float(np.sqrt(t * t + 1.0))
                s = t * c
                for k in range(6):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p] = c * akp - s * akq
                    a[k][q] = s * akp + c * akq
                for k in range(6):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k] = c * apk - s * aqk
                    a[q][k] = s * apk + c * aqk
                for k in range(6):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - s * vkq
                    v[k][q] = s * vkp + c * vkq
        if not rotated:
            break
    return np.array([a[k][k] for k in range(6)]), np.array(v)


def solve_normal(ata, atb):
    """Minimum-norm solution of the normal equations: eigenvalues <= 1e-12 * the largest are taken as 0."""
    lam, v = jacobi6(ata)
    lmax = max(0.0, float(lam.max()))
    x = [0.0] * 6
    for k in range(6):
        if not lam[k] > EIG_REL * lmax:
            continue
        d = 0.0
        for r in range(6):
            d += float(v[r, k]) * float(atb[r])
        cf = d / float(lam[k])
        for r in range(6):
            x[r] += cf * float(v[r, k])
    return np.array(x)


def point_to_plane_system(P, Q):
    """Rows A = [p x n_q, n_q], b = (q - p) . n_q of matched float32 rows P[k], Q[k] (float64)."""
    p = P[:, :3].astype(np.float64)
    q = Q[:, :3].astype(np.float64)
    n = Q[:, 3:6].astype(np.float64)
    A = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0],
                  n[:, 0], n[:, 1], n[:, 2]], axis=1)
    b = ((q[:, 0] - p[:, 0]) * n[:, 0] + (q[:, 1] - p[:, 1]) * n[:, 1]) + (q[:, 2] - p[:, 2]) * n[:, 2]
    return A, b


def transform_mat(x):
    """getTransformMat: [Rz(x2) Ry(x1) Rx(x0) | x3..5]."""
    ct, st, cp, sp, cy, sy = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    X = np.eye(4)
    X[0, :] = [cy * cp, cy * sp * st - sy * ct, cy * sp * ct + sy * st, x[3]]
    X[1, :] = [sy * cp, sy * sp * st + cy * ct, sy * sp * ct - cy * st, x[4]]
    X[2, :] = [-sp, cp * st, cp * ct, x[5]]
    return X


def matmul4(A, B):
    """4 x 4 float64 product summed k = 0..3 in order (the kernels' order)."""
    r = np.zeros((4, 4))
    for a in range(4):
        for b in range(4):
            s = A[a, 0] * B[0, b]
            for k in range(1, 4):
                s = s + A[a, k] * B[k, b]
            r[a, b] = s
    return r


def icp(S, T, max_iterations=100, tolerance=0.005, rejection_scale=2.5, num_levels=2, nearest=None):
    """registerModelToScene(S, T) as DESIGN.md 8.2 states it.  Returns a dict: status (0 or -3 for a non-finite xyz), pose (4 x 4),
    iterations / pairs / fval_min per level (index = level), scale, mean_avg.  nearest(Q) -> callable M -> (j, d2) (default: kd-tree
    candidates + the float32 rule; nearest_brute-based for cross-checks)."""
    S = np.asarray(S, F32).reshape(-1, 6)
    T = np.asarray(T, F32).reshape(-1, 6)
    n, m = len(S), len(T)
    L = num_levels
    res = dict(status=0, pose=np.eye(4), iterations=[0] * 8, pairs=[0] * 8, fval_min=[0.0] * 8, scale=0.0, mean_avg=np.zeros(3))
    if not (np.isfinite(S[:, :3]).all() and np.isfinite(T[:, :3]).all()):
        res["status"] = -3
        return res
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s0, t0, mean_avg, scale = normalise(S, T)
    if not (np.isfinite(F32(scale)) and F32(scale) > 0):       # every point at the mean: no finite normalisation
        res["status"] = -3
        return res
    pose = np.eye(4)
    for level in range(L - 1, -1, -1):
        c = level_constants(n, m, level, max_iterations, tolerance)
        step, tolp, max_it = c["step"], c["tolp"], c["max_it"]
        P = transform(pose, s0[0:c["np"] * step:step])
        Q = t0[0:c["nq"] * step:step]
        fval_old = fval_min = FVAL_INIT
        fval_perc = 0.0
        X = np.eye(4)
        it = pairs = 0
        if len(Q):
            nn = (nearest or NearestQ)(Q)
            M = P[:, :3].copy()
            while not (fval_perc < 1 + tolp and fval_perc > 1 - tolp) and it < max_it:
                j, d2 = nn(M)
                keep = reject(d2, rejection_scale)
                pi, pj = picky(j, d2, keep)
                pairs = len(pi)
                if pairs < 6:
                    break
                A, b = point_to_plane_system(P[pi], Q[pj])
                x = solve_normal(A.T @ A, A.T @ b)
                if np.isnan(x).any():
                    break
                X = transform_mat(x)
                M = transform(X, P, normals=False)
                diff = P[pi].astype(np.float64) - Q[pj].astype(np.float64)
                fval = np.sqrt(np.sum(diff * diff)) / len(P)
                fval_perc = fval / fval_old
                fval_old = fval
                if fval < fval_min:
                    fval_min = fval
                it += 1
        pose = matmul4(X, pose)
        res["iterations"][level], res["pairs"][level], res["fval_min"][level] = it, pairs, fval_min
    R = pose[:3, :3]
    for r in range(3):
        rm = (R[r, 0] * mean_avg[0] + R[r, 1] * mean_avg[1]) + R[r, 2] * mean_avg[2]
        pose[r, 3] = (pose[r, 3] / scale + mean_avg[r]) - rm
    res.update(pose=pose, scale=scale, mean_avg=mean_avg)
    return res


def refined_pose(icp_pose, R_job, t_adjusted_mm):
    """icp_refinement :91-93 and icp3d.py :466-467: tf = pose * [R | t_adjusted / 1000]; R_ref = tf[:3,:3], t_ref = tf[:3,3] * 1000."""
    tf = np.eye(4)
    tf[:3, :3] = np.asarray(R_job, np.float64).reshape(3, 3)
    tf[:3, 3] = np.asarray(t_adjusted_mm, np.float64) / 1000.0
    tf = matmul4(np.asarray(icp_pose, np.float64), tf)
    return tf[:3, :3].copy(), tf[:3, 3] * 1000.0


def rotation_error_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra).T @ np.asarray(Rb)) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
