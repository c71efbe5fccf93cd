"""float64 numpy restatement of depth back-projection, normals and the ICP point sets (pix2pose_amd/csrc/normals.hip, DESIGN.md
section 8), for the tests only.  Every rule below is the kernel's, expression by expression (same operand order, no fused
multiply-add); the reference lines each one restates are named in DESIGN.md 8.

    inpaint(d)           the onion-peel stand-in for cv2.inpaint(d32, d == 0, 2, INPAINT_NS), FILL_LAYERS layers
    gaussian(f)          ndimage.gaussian_filter(f, 2) on float64 (separable, radius 8, mode 'reflect')
    gradient(f, axis)    np.gradient(f, 2, edge_order=2) along one axis
    get_xyz / get_normal getXYZ / get_normal(refine=True), with or without a bbox crop
    scene_points(d, K)   points_tgt of icp3d.py:372-374: float32 [H, W, 6]
    icp_inputs(...)      icp_refinement :58-85 up to registerModelToScene, given the scene points and a renderer
"""
import math

import numpy as np

FILL_LAYERS = 10
GAUSS_R = 8
NAN32 = np.float32(np.nan)


def inpaint(d, layers=FILL_LAYERS):
    """Onion-peel fill.  Known pixels: nan_to_num(d) != 0.  Layer k = 1..layers fills every unknown pixel with a known 8-neighbour
    (known = as after layer k - 1) with the mean of the known pixels of its 5 x 5 window, summed in float64 in row-major window
    order and rounded to float32; the window is clipped to the image.  Pixels still unknown after the last layer are 0."""
    v = np.nan_to_num(np.asarray(d, np.float32)).astype(np.float32)
    H, W = v.shape
    f = np.where(v != 0, v, NAN32).astype(np.float32)
    for _ in range(layers):
        known = ~np.isnan(f)
        kp = np.pad(known, 1)
        near = np.zeros_like(known)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                near |= kp[1 + dr:1 + dr + H, 1 + dc:1 + dc + W]
        todo = ~known & near
        fp = np.pad(np.where(known, f, 0).astype(np.float64), 2)
        kp2 = np.pad(known, 2)
        s = np.zeros((H, W))
        n = np.zeros((H, W), np.int64)
        for dr in range(-2, 3):
            for dc in range(-2, 3):
                s = s + np.where(kp2[2 + dr:2 + dr + H, 2 + dc:2 + dc + W], fp[2 + dr:2 + dr + H, 2 + dc:2 + dc + W], 0.0)
                n += kp2[2 + dr:2 + dr + H, 2 + dc:2 + dc + W]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = (s / n).astype(np.float32)
        f = np.where(todo, mean, f).astype(np.float32)
    return np.where(np.isnan(f), np.float32(0), f).astype(np.float32)


def gauss_weights():
    """scipy's _gaussian_kernel1d(2, 0, 8): exp(-0.5 / 4 x^2), normalised by their sum (summed x = -8 .. 8); centre first."""
    phi = [math.exp(-0.5 / 4.0 * float(x * x)) for x in range(-GAUSS_R, GAUSS_R + 1)]
    s = 0.0
    for p in phi:
        s += p
    return [phi[GAUSS_R + k] / s for k in range(GAUSS_R + 1)]


def reflect_index(i, n):
    """'reflect' (d c b a | a b c d), repeated with period 2n for lines shorter than the radius."""
    m = np.mod(i, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def _correlate(f, axis, w):
    f = np.moveaxis(np.asarray(f, np.float64), axis, 0)
    n = f.shape[0]
    idx = np.arange(n)
    acc = f * w[0]
    for k in range(GAUSS_R, 0, -1):
        acc = acc + (f[reflect_index(idx - k, n)] + f[reflect_index(idx + k, n)]) * w[k]
    return np.moveaxis(acc, 0, axis)


def gaussian(f):
    """ndimage.gaussian_filter(f, 2): axis 0, then axis 1; correlate1d's symmetric loop x[0] w[0] + sum_{k=8..1} (x[-k] + x[k]) w[k]."""
    w = gauss_weights()
    return _correlate(_correlate(f, 0, w), 1, w)


def gradient(f, axis):
    """np.gradient(f, 2, edge_order=2) along `axis`: interior (f[i+1] - f[i-1]) / 4; edges -0.75 f0 + 1.0 f1 + -0.25 f2 and
    0.25 f[n-3] + -1.0 f[n-2] + 0.75 f[n-1] (numpy's coefficients for uniform spacing 2)."""
    f = np.moveaxis(np.asarray(f, np.float64), axis, 0)
    out = np.empty_like(f)
    out[1:-1] = (f[2:] - f[:-2]) / 4.0
    out[0] = -0.75 * f[0] + 1.0 * f[1] + -0.25 * f[2]
    out[-1] = 0.25 * f[-3] + -1.0 * f[-2] + 0.75 * f[-1]
    return np.moveaxis(out, 0, axis)


def uv_offsets(H, W, K):
    """The reference's int16 uv_table: (u - cx) and (v - cy) truncated toward zero; the skew K[0, 1] is not used."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    uu = np.trunc(np.arange(W) - K[0, 2]).astype(np.float64)
    vv = np.trunc(np.arange(H) - K[1, 2]).astype(np.float64)
    return np.broadcast_to(uu[None, :], (H, W)), np.broadcast_to(vv[:, None], (H, W))


def _crop(a, bbox):
    return a if bbox is None else a[bbox[0]:bbox[2], bbox[1]:bbox[3]]


def get_xyz(depth, K, bbox=None):
    """getXYZ: x = (u - cx)_int16 * d / fx, y = (v - cy)_int16 * d / fy, z = d, in float64 (the caller stores float32)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    d = np.asarray(depth, np.float32)
    uu, vv = uv_offsets(*d.shape, K)
    d = _crop(d, bbox).astype(np.float64)
    uu, vv = _crop(uu, bbox), _crop(vv, bbox)
    return np.stack([uu * d / K[0, 0], vv * d / K[1, 1], d], -1)


def get_normal(depth, K, bbox=None, layers=FILL_LAYERS):
    """get_normal(refine=True): fill, Gaussian over the WHOLE image, crop, gradient of the crop, cross(v_x, v_y) / |.| (0 -> 1),
    nan_to_num; float64."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    d = np.asarray(depth, np.float32)
    uu, vv = uv_offsets(*d.shape, K)
    s = _crop(gaussian(inpaint(d, layers).astype(np.float64)), bbox)
    uu, vv = _crop(uu, bbox), _crop(vv, bbox)
    gy, gx = gradient(s, 0), gradient(s, 1)
    kx, ky = 1.0 / K[0, 0], 1.0 / K[1, 1]
    vy0, vy1, vy2 = uu * kx * gy, s * ky + vv * ky * gy, gy
    vx0, vx1, vx2 = s * kx + uu * kx * gx, vv * ky * gx, gx
    c0, c1, c2 = vx1 * vy2 - vx2 * vy1, vx2 * vy0 - vx0 * vy2, vx0 * vy1 - vx1 * vy0
    nrm = np.sqrt(c0 * c0 + c1 * c1 + c2 * c2)
    nrm = np.where(nrm == 0, 1.0, nrm)
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(np.stack([c0 / nrm, c1 / nrm, c2 / nrm], -1))


def points(depth, K, bbox=None, layers=FILL_LAYERS):
    """float32 [h, w, 6] = getXYZ | get_normal over the image or the bbox crop."""
    with np.errstate(invalid="ignore"):
        return np.concatenate([get_xyz(depth, K, bbox), get_normal(depth, K, bbox, layers)], -1).astype(np.float32)


def scene_points(depth, K, layers=FILL_LAYERS):
    """points_tgt of icp3d.py:372-374."""
    return points(depth, K, None, layers)


def bbox_from_mask(mask):
    """get_bbox_from_mask: [rmin, cmin, rmax, cmax], max INCLUSIVE; zeros for an empty mask."""
    vu = np.where(mask)
    if len(vu[0]) == 0:
        return np.zeros(4, np.int64)
    return np.array([vu[0].min(), vu[1].min(), vu[0].max(), vu[1].max()], np.int64)


def centroid(p):
    """float64 mean of float32 xyz (NaN for no points)."""
    p = np.asarray(p, np.float32).reshape(-1, 6)[:, :3].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return p.sum(0) / len(p)


def icp_inputs(scene_pts, union_mask, t_mm, K, render, layers=FILL_LAYERS):
    """icp_refinement :58-85 up to registerModelToScene.  render(t_mm) -> the float32 [H, W] depth of the job at t (mm).
    Returns dict(status 0 / -1 (bbox) / -2 (count), bbox, t_init, t_adjusted, centroid_src, centroid_tgt, src, tgt)."""
    union_mask = np.asarray(union_mask) != 0
    tgt = scene_pts[union_mask]
    ctgt = centroid(tgt)
    t = np.asarray(t_mm, np.float64).copy()
    if t[2] < 300 or t[2] > 5000:
        t = ctgt * 1000.0
    depth_init = np.asarray(render(t), np.float32)
    init_mask = (depth_init > 0) & union_mask
    bbox = bbox_from_mask(init_mask)
    res = {"bbox": bbox.tolist(), "t_init": t, "t_adjusted": t.copy(), "centroid_src": np.zeros(3), "centroid_tgt": ctgt,
           "src": np.zeros((0, 6), np.float32), "tgt": tgt}
    if bbox[2] - bbox[0] < 5 or bbox[3] - bbox[1] < 5:
        return dict(res, status=-1)
    if init_mask.sum() < 10:
        return dict(res, status=-2)
    src = points(depth_init, K, bbox, layers)[init_mask[bbox[0]:bbox[2], bbox[1]:bbox[3]]]
    csrc = centroid(src)
    adj = ctgt - csrc
    src = src.copy()
    src[:, :3] = (src[:, :3].astype(np.float64) + adj).astype(np.float32)
    return dict(res, status=0, t_adjusted=t + adj * 1000.0, centroid_src=csrc, src=src)
