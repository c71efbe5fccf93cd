"""float64 numpy restatement of the XYZ colour render (pix2pose_amd/csrc/depth.hip: p2p_render_xyz_batch)
and of the patch rules of the reference's tools/2_2_render_pix2pose_training.py:168-184, for the tests only.  Geometry comes from
depth_ref: render_xyz() draws the triangles of depth_ref.render_depth() in index order and keeps, per pixel, the nearest float32
depth and, among equal depths, the first (lowest) triangle index -- GL_LESS.

raycast_color() is an oracle that does not share the colour derivation: it intersects the pixel's ray with the owning triangle in
camera space and takes the 3-D barycentrics of the hit point, where render_xyz() interpolates c / z and 1 / z in screen space.
"""
import numpy as np

import depth_ref as D


def vertex_colors(colors_u8):
    """p2p_mesh_set_colors / Model3D.load: float32(c) / 255 in float32."""
    return np.asarray(colors_u8, np.uint8).astype(np.float32) / np.float32(255)


def render_xyz(verts_mm, tris, colors_u8, K, R, t, H, W):
    """t in mm.  -> color float32 [H,W,3] (0 = empty), depth float32 [H,W], owner int [H,W] (triangle index, -1 = empty),
    margin bool [H,W] (centres within 1e-4 px of an edge of a drawn triangle, as depth_ref.render_depth marks them)."""
    u, v, zc = D.project(verts_mm, K, R, t)
    col = vertex_colors(colors_u8).astype(np.float64)
    zbuf = np.full((H, W), np.inf, np.float32)
    color = np.zeros((H, W, 3), np.float32)
    owner = np.full((H, W), -1, np.int64)
    margin = np.zeros((H, W), bool)
    for fi, f in enumerate(np.asarray(tris).reshape(-1, 3)):
        if not np.all(zc[f] >= D.CLIP_NEAR):
            continue
        uu, vv, zz, cc = u[f].copy(), v[f].copy(), zc[f].copy(), col[f].copy()
        if not np.all((np.abs(uu) < 1e9) & (np.abs(vv) < 1e9)):
            continue
        area = (uu[1] - uu[0]) * (vv[2] - vv[0]) - (uu[2] - uu[0]) * (vv[1] - vv[0])
        if not area < 0:
            continue
        uu, vv, zz, cc = uu[[0, 2, 1]], vv[[0, 2, 1]], zz[[0, 2, 1]], cc[[0, 2, 1]]
        A = -area
        i0, i1 = int(max(0.0, np.ceil(uu.min() - 0.5))), int(min(W - 1.0, np.floor(uu.max() - 0.5)))
        j0, j1 = int(max(0.0, np.ceil(vv.min() - 0.5))), int(min(H - 1.0, np.floor(vv.max() - 0.5)))
        if i0 > i1 or j0 > j1:
            continue
        pu, pv = np.meshgrid(np.arange(i0, i1 + 1) + 0.5, np.arange(j0, j1 + 1) + 0.5)
        bs, ins = [], np.ones(pu.shape, bool)
        loose, near = np.ones(pu.shape, bool), np.zeros(pu.shape, bool)
        for a, b in ((1, 2), (2, 0), (0, 1)):
            du, dv = uu[b] - uu[a], vv[b] - vv[a]
            e = du * (pv - vv[a]) - dv * (pu - uu[a])
            bs.append(e / A)
            ins &= D._edge_in(e, du, dv)
            tol = 1e-4 * np.hypot(du, dv)
            loose &= e >= -tol
            near |= np.abs(e) <= tol
        iz = bs[0] / zz[0] + bs[1] / zz[1] + bs[2] / zz[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            d = 1.0 / iz
            c = np.stack([((bs[0] * cc[0, k]) / zz[0] + (bs[1] * cc[1, k]) / zz[1] + (bs[2] * cc[2, k]) / zz[2]) / iz
                          for k in range(3)], -1)
        ok = ins & (d >= D.CLIP_NEAR) & (d <= D.CLIP_FAR)
        d32 = np.where(ok, d, np.inf).astype(np.float32)
        sub = zbuf[j0:j1 + 1, i0:i1 + 1]
        win = d32 < sub                       # strict: an equal depth keeps the earlier (lower) triangle
        sub[win] = d32[win]
        color[j0:j1 + 1, i0:i1 + 1][win] = c[win].astype(np.float32)
        owner[j0:j1 + 1, i0:i1 + 1][win] = fi
        margin[j0:j1 + 1, i0:i1 + 1] |= loose & near
    depth = np.where(np.isinf(zbuf), np.float32(0), zbuf)
    return color, depth, owner, margin


def raycast_color(verts_mm, tris, colors_u8, K, R, t_mm, owner):
    """The colour of every owned pixel by another route: the ray K^-1 (i + 0.5, j + 0.5, 1) is intersected with the plane of triangle
    owner[j, i] in camera space, and the colour is the 3-D barycentric mix of the hit point (areas of the sub-triangles through
    cross products).  -> (color float64 [H,W,3] (0 where owner < 0), hit float64 [H,W,3]: the hit point in camera space, metres)."""
    V = D.mesh_metres(verts_mm).astype(np.float64)
    pose = D.gl_pose(t_mm, R)
    Vc = V @ pose[:3, :3].T + pose[:3, 3]
    col = vertex_colors(colors_u8).astype(np.float64)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    H, W = owner.shape
    jj, ii = np.nonzero(owner >= 0)
    f = tris[owner[jj, ii]]
    a, b, c = Vc[f[:, 0]], Vc[f[:, 1]], Vc[f[:, 2]]
    rays = np.linalg.solve(np.asarray(K, np.float64).reshape(3, 3), np.stack([ii + 0.5, jj + 0.5, np.ones(len(ii))])).T
    n = np.cross(b - a, c - a)
    s = np.einsum("ij,ij->i", n, a) / np.einsum("ij,ij->i", n, rays)
    P = rays * s[:, None]
    nn = np.einsum("ij,ij->i", n, n)
    wa = np.einsum("ij,ij->i", np.cross(b - P, c - P), n) / nn
    wb = np.einsum("ij,ij->i", np.cross(c - P, a - P), n) / nn
    wc = np.einsum("ij,ij->i", np.cross(a - P, b - P), n) / nn
    out = np.zeros((H, W, 3))
    out[jj, ii] = wa[:, None] * col[f[:, 0]] + wb[:, None] * col[f[:, 1]] + wc[:, None] * col[f[:, 2]]
    hit = np.zeros((H, W, 3))
    hit[jj, ii] = P
    return out, hit


def bbox_of(depth):
    """get_rendering (2_2:61-62): [min v, min u, max v, max u] of depth > 0, max inclusive; [-1] * 4 for an empty render (where
    the reference raises)."""
    vv, uu = np.nonzero(np.asarray(depth) > 0)
    if len(vv) == 0:
        return np.array([-1, -1, -1, -1])
    return np.array([vv.min(), uu.min(), vv.max(), uu.max()])


def quant_table():
    """What 2_2 stores for a colour the GL buffer holds as the 8-bit level q: the read-back is float32(q) / 255 in float32,
    get_rendering multiplies by 255 in float32, and the assignment into the uint8 patch truncates.  -> uint8 [256]."""
    q = np.arange(256, dtype=np.float32)
    return ((q / np.float32(255)) * np.float32(255)).astype(np.uint8)


def quantise(color):
    """float colour in [0, 1] -> the uint8 the reference's patch holds: q = floor(c * 255 + 0.5), then quant_table()[q]."""
    q = np.floor(np.asarray(color, np.float64) * 255 + 0.5).astype(np.int64)
    return quant_table()[np.clip(q, 0, 255)]


def patch_unresized(rgb_u8, color, depth, bbox):
    """2_2:168-171: -> uint8 [h,w,6], rgb with [128,128,128] where depth == 0, xyz quantised, cropped to bbox[0]:bbox[2],
    bbox[1]:bbox[3] -- the box's max is inclusive, so the slice leaves the last covered row and column out.  None when the render
    is empty or the box has a zero side."""
    b = [int(x) for x in bbox]
    if b[2] < 0 or b[2] - b[0] == 0 or b[3] - b[1] == 0:
        return None
    img = np.array(rgb_u8, np.uint8)
    img[np.asarray(depth) == 0] = [128, 128, 128]
    data = np.zeros((b[2] - b[0], b[3] - b[1], 6), np.uint8)
    data[:, :, :3] = img[b[0]:b[2], b[1]:b[3]]
    data[:, :, 3:] = quantise(color)[b[0]:b[2], b[1]:b[3]]
    return data


def patch_shape(h, w):
    """2_2:172-177: the stored patch's (h, w): unchanged when max(h, w) <= 128, else int(h * scale + 0.5), int(w * scale + 0.5)
    with scale = 128.0 / max(h, w)."""
    m = max(h, w)
    if m <= 128:
        return h, w
    scale = 128.0 / m
    return int(h * scale + 0.5), int(w * scale + 0.5)


def patch(rgb_u8, color, depth, bbox, gen=0):
    """2_2:168-184 whole: patch_unresized(), and when its longer side exceeds 128 each half resized on its own by
    skimage.transform.resize of generation gen as oracle.est_pose_oracle restates it (default arguments: <= 0.14 'constant' mode
    without anti-aliasing, later generations 'reflect' with it), acting on float32(x / 255); times 255, truncated."""
    from oracle import est_pose_oracle as O
    data = patch_unresized(rgb_u8, color, depth, bbox)
    if data is None:
        return None
    oh, ow = patch_shape(*data.shape[:2])
    if (oh, ow) == data.shape[:2]:
        return data
    if oh == 0 or ow == 0:
        return None
    new = np.zeros((oh, ow, 6), np.uint8)
    mode = "constant" if gen == 0 else "reflect"
    for s in (slice(0, 3), slice(3, 6)):
        new[:, :, s] = (O.resize_gen((data[:, :, s] / 255).astype(np.float32), (oh, ow), mode, 0.0, gen) * 255).astype(np.uint8)
    return new
