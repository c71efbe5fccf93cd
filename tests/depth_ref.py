"""float64 numpy restatement of the depth path (pix2pose_amd/csrc/depth.hip), for the tests only.

render_depth() follows the rules of p2p_render_depth_batch expression by expression (same operand order, no fused
multiply-add), so where both cover a pixel the two depths agree to the last float32 bit but for the rare rounding tie;
depth_score() restates icp3d.py:470-490.  Also the synthetic meshes the tests draw.
"""
import numpy as np

CLIP_NEAR, CLIP_FAR = 0.01, 10.0


def mesh_metres(verts_mm):
    """Model3D.load(scale=0.001): a float32 cloud times 0.001 in float32."""
    return np.asarray(verts_mm, np.float32) * np.float32(0.001)


def pose_metres(t_mm):
    """t of a p2p_refine_job (mm) -> what the rasteriser uses: render_obj(..., tra_pred/1000, ...), then its quirk
    if(tra[2]>100): tra = tra/1000 (icp3d.py:46)."""
    t = np.asarray(t_mm, np.float64) / 1000.0
    return t / 1000.0 if t[2] > 100.0 else t


def _edge_in(e, du, dv):
    return (e > 0) | ((e == 0) & ((dv > 0) | ((dv == 0) & (du < 0))))


def render_depth(verts_mm, tris, K, R, t, H, W, with_margin=False, with_counts=False):
    """t in mm.  -> depth float32 [H,W] (metres, 0 = empty); with_margin=True also a bool [H,W] of pixel centres that lie within
    1e-4 px of an edge of a drawn triangle (where a float rounding may flip coverage); with_counts=True (instead) an int [H,W]
    of how many drawn triangles cover each centre."""
    V = mesh_metres(verts_mm).astype(np.float64)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = pose_metres(t)
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    X, Y, Z = V[:, 0], V[:, 1], V[:, 2]
    xc = R[0, 0] * X + R[0, 1] * Y + R[0, 2] * Z + t[0]
    yc = R[1, 0] * X + R[1, 1] * Y + R[1, 2] * Z + t[1]
    zc = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z + t[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * (xc / zc) + s * (yc / zc) + cx
        v = fy * (yc / zc) + cy
    zbuf = np.full((H, W), np.inf, np.float32)
    margin = np.zeros((H, W), bool)
    counts = np.zeros((H, W), np.int64)
    for f in np.asarray(tris).reshape(-1, 3):
        if not np.all(zc[f] >= CLIP_NEAR):
            continue
        uu, vv, zz = u[f].copy(), v[f].copy(), zc[f].copy()
        if not np.all((np.abs(uu) < 1e9) & (np.abs(vv) < 1e9)):
            continue
        area = (uu[1] - uu[0]) * (vv[2] - vv[0]) - (uu[2] - uu[0]) * (vv[1] - vv[0])
        if not area < 0:
            continue
        uu, vv, zz = uu[[0, 2, 1]], vv[[0, 2, 1]], zz[[0, 2, 1]]
        A = -area
        i0, i1 = int(max(0.0, np.ceil(uu.min() - 0.5))), int(min(W - 1.0, np.floor(uu.max() - 0.5)))
        j0, j1 = int(max(0.0, np.ceil(vv.min() - 0.5))), int(min(H - 1.0, np.floor(vv.max() - 0.5)))
        if i0 > i1 or j0 > j1:
            continue
        pu, pv = np.meshgrid(np.arange(i0, i1 + 1) + 0.5, np.arange(j0, j1 + 1) + 0.5)
        es, ins = [], np.ones(pu.shape, bool)
        loose, near = np.ones(pu.shape, bool), np.zeros(pu.shape, bool)
        for a, b in ((1, 2), (2, 0), (0, 1)):
            du, dv = uu[b] - uu[a], vv[b] - vv[a]
            e = du * (pv - vv[a]) - dv * (pu - uu[a])
            es.append(e)
            ins &= _edge_in(e, du, dv)
            tol = 1e-4 * np.hypot(du, dv)       # e / |edge| is the distance to the edge's line in px
            loose &= e >= -tol
            near |= np.abs(e) <= tol
        iz = (es[0] / A) / zz[0] + (es[1] / A) / zz[1] + (es[2] / A) / zz[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            d = 1.0 / iz
        ok = ins & (d >= CLIP_NEAR) & (d <= CLIP_FAR)
        sub = zbuf[j0:j1 + 1, i0:i1 + 1]
        np.minimum(sub, np.where(ok, d, np.inf).astype(np.float32), out=sub)
        if with_margin:
            margin[j0:j1 + 1, i0:i1 + 1] |= loose & near       # centres within 1e-4 px of the triangle's boundary
        counts[j0:j1 + 1, i0:i1 + 1] += ok
    depth = np.where(np.isinf(zbuf), np.float32(0), zbuf)
    if with_counts:
        return depth, counts
    return (depth, margin) if with_margin else depth


def depth_score(depth_ref, depth_t, union_mask):
    """icp3d.py:470-490 and fcn() at :314-315."""
    m = np.asarray(union_mask) != 0
    diff = np.abs(depth_ref[m].astype(np.float64) - depth_t[m].astype(np.float64))
    inl = diff < 0.02
    inlier_mask = np.zeros(m.shape, bool)
    inlier_mask[m] = inl
    union = int(m.sum())
    return {"inlier_count": int(inl.sum()), "union": union, "fcn": float(np.sum(np.maximum(0, 0.02 - diff) / 0.02)),
            "ratio": float(inl.sum()) / union if union else 0.0}, inlier_mask


def box_mesh(lo, hi, n=8):
    """Closed axis-aligned box [lo, hi] (mm), every face an n x n grid of quads split into triangles, wound counter-clockwise
    seen from outside (outward normals by the right-hand rule)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    verts, tris = [], []
    for ax in range(3):
        for side in (0, 1):
            a, b = (ax + 1) % 3, (ax + 2) % 3
            base = len(verts)
            g = np.linspace(0, 1, n + 1)
            for ia in g:
                for ib in g:
                    p = np.empty(3)
                    p[ax] = hi[ax] if side else lo[ax]
                    p[a] = lo[a] + ia * (hi[a] - lo[a])
                    p[b] = lo[b] + ib * (hi[b] - lo[b])
                    verts.append(p)
            for ia in range(n):
                for ib in range(n):
                    q = [base + ia * (n + 1) + ib, base + (ia + 1) * (n + 1) + ib, base + (ia + 1) * (n + 1) + ib + 1,
                         base + ia * (n + 1) + ib + 1]
                    # (a, b, ax) is right-handed: a-then-b is counter-clockwise seen from +ax
                    if side == 0:
                        q = q[::-1]
                    tris += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return np.array(verts), np.array(tris, np.int64)


def l_mesh(n=8):
    """Asymmetric L-shaped extrusion (mm): two overlapping closed boxes, outward winding, 2 x 6 x 2 n^2 triangles."""
    v1, t1 = box_mesh([-40, -30, -15], [40, -5, 15], n)
    v2, t2 = box_mesh([-40, -30, -15], [-15, 45, 15], n)
    return np.concatenate([v1, v2]), np.concatenate([t1, t2 + len(v1)])


def rot(ax, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][ax]
    R = np.eye(3)
    R[i, i] = c; R[j, j] = c; R[i, j] = -s; R[j, i] = s
    return R


K_640 = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def pixel_grid_mesh():
    """A flat 4 x 4-quad square at z = 0 whose vertices land EXACTLY on pixel centres under GRID_K at t = (0, 0, 1000) mm:
    vertex coordinates are multiples of 250 mm, float32(250 k) * float32(0.001) rounds to k / 4 exactly for |k| <= 2, so
    u = 64 * k / 4 + 320.5 is a pixel centre.  Every shared and every outer edge runs through centres, so the tie rule decides
    them all.  Quads are split along alternating diagonals and wound so that the camera sees their front."""
    ks = np.arange(-2, 3) * 250.0
    verts = np.array([(x, y, 0.0) for y in ks for x in ks])
    tris = []
    for a in range(4):
        for b in range(4):
            q = [a * 5 + b, a * 5 + b + 1, (a + 1) * 5 + b + 1, (a + 1) * 5 + b]
            if (a + b) % 2:
                tris += [(q[0], q[2], q[1]), (q[0], q[3], q[2])]
            else:
                tris += [(q[0], q[3], q[1]), (q[1], q[3], q[2])]
    return verts, np.array(tris)


GRID_K = np.array([[64.0, 0.0, 320.5], [0.0, 64.0, 240.5], [0.0, 0.0, 1.0]])
