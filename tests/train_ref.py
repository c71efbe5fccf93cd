"""numpy / scipy restatement of the reference's pix2pose_util/data_io.py: get_patch_pair (:53-274) for scikit-image 0.17 / 0.18, from
explicit draw records (runtime.train_draws), and of the colour stage's records (runtime.train_colours); for the tests only.
DESIGN.md section 8.5.  tests/test_train_batch_cpu.py holds it to the recorded outputs of the real function within 1e-9.

Each array keeps the dtype the reference gives it: the patch, the background and the composited images are float32 (and the image
blur is scipy's float32 filter, rounded per axis pass), xyz / c_img, the masks as float, base_image and everything behind the
normalisation are float64.  skimage.filters.gaussian is scipy.ndimage.gaussian_filter(mode='nearest', truncate=4.0) with sigma 0 on
the channel axis; resize is oracle.est_pose_oracle.resize_gen; rotate without resize is the float64 warp written out below.
"""
import numpy as np
from scipy import ndimage as ndi

from oracle import est_pose_oracle as O

f32 = np.float32


def _gaussian(a, sigma):
    a = np.asarray(a)
    return ndi.gaussian_filter(a, [sigma, sigma] + [0] * (a.ndim - 2), mode="nearest", truncate=4.0)


def frame(back_u8, patch_shape):
    """The float32 frame: the background over 255, grey replicated, enlarged by the rule of :78-85."""
    b = np.asarray(back_u8)
    if b.ndim != 3:
        b = np.dstack([b, b, b])
    b = b.astype(f32) / 255
    ph, pw = patch_shape[:2]
    H, W = b.shape[:2]
    if H < 2 * ph or W < 2 * pw:
        b = O.resize_gen(b, (max(2 * ph if H < 2 * ph else 0, H), max(2 * pw if W < 2 * pw else 0, W)), "reflect", 0.0, 1)
        assert b.dtype == np.float32
    return b


def apply_colour(real255, rec, noise=None):
    """The colour stage on the float32 0 .. 255 patch [h, w, 3]: the eight augmenters in rec['order'], clipped to [0, 255] after
    each; the blur is scipy's filter with mirrored edges.  noise: the standard normals [h, w, 3] to use when rec['noise_scale'] > 0."""
    x = np.array(real255, f32)
    for ident in rec["order"]:
        if ident < 3:
            x[..., ident] = x[..., ident] + f32(rec["add"][ident])
        elif ident == 3:
            x = f32(128) + f32(rec["contrast"]) * (x - f32(128))
        elif ident == 4:
            x = x * np.array(rec["mul"], f32)
        elif ident == 5:
            s = float(f32(rec["blur_sigma"]))
            if int(4.0 * s + 0.5) > 0:
                x = ndi.gaussian_filter(x, [s, s, 0], mode="mirror", truncate=4.0)
        elif ident == 6:
            if rec["noise_scale"] > 0:
                assert noise is not None, "the device's noise is not restated: pass the normals"
                x = x + f32(rec["noise_scale"]) * np.asarray(noise, f32)
        else:
            x = f32(128) + np.array(rec["contrast2"], f32) * (x - f32(128))
        x = np.clip(x, f32(0), f32(255)).astype(f32)
    return x


def _warp_f64(img, m, mode):
    """_warp_fast[float64] of one plane onto its own shape: m rows 0 and 1 map (x, y, 1) to (column, row)."""
    n_r, n_c = img.shape
    y, x = np.meshgrid(np.arange(n_r, dtype=np.float64), np.arange(n_c, dtype=np.float64), indexing="ij")
    c = m[0] * x + m[1] * y + m[2]
    r = m[3] * x + m[4] * y + m[5]
    fr, fc = np.floor(r), np.floor(c)
    minr, minc, maxr, maxc = fr.astype(np.int64), fc.astype(np.int64), np.ceil(r).astype(np.int64), np.ceil(c).astype(np.int64)
    dr, dc = r - fr, c - fc

    def px(rr, cc):
        if mode == "reflect":
            return img[O._map_reflect(rr, n_r), O._map_reflect(cc, n_c)]
        ok = (rr >= 0) & (rr < n_r) & (cc >= 0) & (cc < n_c)
        return np.where(ok, img[np.clip(rr, 0, n_r - 1), np.clip(cc, 0, n_c - 1)], 0.0)
    top = (1 - dc) * px(minr, minc) + dc * px(minr, maxc)
    bottom = (1 - dc) * px(maxr, minc) + dc * px(maxr, maxc)
    return (1 - dr) * top + dr * bottom


def rotate(img, m, mode):
    """skimage.transform.rotate(img, angle, mode=mode) of a float64 image (no resize, cval 0, clip=True) given the matrix."""
    img = np.asarray(img, np.float64)
    planes = img[..., None] if img.ndim == 2 else img
    out = np.dstack([_warp_f64(np.ascontiguousarray(planes[..., k]), m, mode) for k in range(planes.shape[2])])
    out = np.clip(out, img.min(), img.max())         # cval 0 lies inside the range of every image rotated here, or mode is 'reflect'
    return out[..., 0] if img.ndim == 2 else out


def get_patch_pair(patch_u8, back_u8, rec, imsize, colour=None, noise=None):
    """-> (src [S, S, 3], tgt [S, S, 3], mask [S, S]) float64.  rec: a record of runtime.train_draws; colour: None or a record of
    runtime.train_colours."""
    imgs = np.asarray(patch_u8).astype(f32)
    real = imgs[:, :, :3] / 255
    p_xyz = imgs[:, :, 3:6] / 255
    ph, pw = p_xyz.shape[:2]
    p_mask = np.sum(p_xyz, axis=2) > 0
    p_xyz[~p_mask] = 0.5
    back = frame(back_u8, (ph, pw))
    assert back.shape[:2] == tuple(rec["frame"])
    aug = real * 255
    if colour is not None:
        aug = apply_colour(aug, colour, noise)
    aug = aug / 255
    assert aug.dtype == np.float32
    v0, u0 = rec["v_ref"], rec["u_ref"]
    aug[~p_mask] = back[v0:v0 + ph, u0:u0 + pw][~p_mask]
    image_ref = back.copy()
    image_ref[v0:v0 + ph, u0:u0 + pw] = aug
    xyz = np.full(back.shape[:2] + (3,), 0.5)
    xyz[v0:v0 + ph, u0:u0 + pw] = p_xyz
    mask_ori = np.zeros(back.shape[:2], bool)
    mask_ori[v0:v0 + ph, u0:u0 + pw] = p_mask

    def rect(k):
        r0, r1, c0, c1 = rec["rect"][k]
        m = np.zeros(back.shape[:2], bool)
        if r0 < r1 and c0 < c1:
            m[r0:r1, c0:c1] = True
        return m
    mask_no_occ = mask_ori & ~rect(0)
    image = back.copy()
    image[mask_no_occ] = image_ref[mask_no_occ]
    win = (slice(rec["v1"], rec["v2"]), slice(rec["u1"], rec["u2"]))
    g = np.gradient(mask_no_occ[win].astype(float))
    boundary = (g[0] > 0) | (g[1] > 0)
    edge = _gaussian(boundary.astype(float), rec["sigma_edge"]) > 0
    blurred = _gaussian(image[win], rec["sigma_blur"])
    assert blurred.dtype == np.float32
    w_img = image[win].copy()
    w_img[edge] = blurred[edge]
    c_img = (xyz - 0.5) / 0.5
    if rec["even"]:
        s = rec["sigma_ran"]
        keep = _gaussian(mask_ori[win].astype(float), s) > 0
        radius = np.linalg.norm(_gaussian(c_img[win], s), axis=2)
        keep &= radius > 0.3
        w_img[~keep] = 0.5
        w_img[rect(1)[win]] = 0.5
        incl = (rect(2) & ~mask_ori)[win]
        w_img[incl] = image_ref[win][incl]
    content = (w_img - np.array([0.5, 0.5, 0.5])) / 0.5
    side, sv, su = rec["side"], rec["shift_v"], rec["shift_u"]
    wh, ww = content.shape[:2]
    base, tgt, msk = np.zeros((side, side, 3)), np.zeros((side, side, 3)), np.zeros((side, side))
    base[sv:sv + wh, su:su + ww] = content
    tgt[sv:sv + wh, su:su + ww] = c_img[win]
    msk[sv:sv + wh, su:su + ww] = mask_ori[win]
    m = np.asarray(rec["rot"], np.float64)
    base, tgt, msk = rotate(base, m, "reflect"), rotate(tgt, m, "reflect"), rotate(msk, m, "constant")
    S = (imsize, imsize)
    return O.resize_gen(base, S, "reflect", 0.0, 1), O.resize_gen(tgt, S, "reflect", 0.0, 1), O.resize_gen(msk, S, "reflect", 0.0, 1)


def radius_margin(patch_u8, rec):
    """Smallest |radius - 0.3| over the window of an even-batch sample (inf otherwise) and smallest non-zero xyz sum distance: what
    the fixture maker's margin assertion measures."""
    if not rec["even"]:
        return np.inf
    imgs = np.asarray(patch_u8).astype(f32)
    p_xyz = imgs[:, :, 3:6] / 255
    p_mask = np.sum(p_xyz, axis=2) > 0
    p_xyz[~p_mask] = 0.5
    Hb, Wb = rec["frame"]
    xyz = np.full((Hb, Wb, 3), 0.5)
    xyz[rec["v_ref"]:rec["v_ref"] + p_xyz.shape[0], rec["u_ref"]:rec["u_ref"] + p_xyz.shape[1]] = p_xyz
    c = ((xyz - 0.5) / 0.5)[rec["v1"]:rec["v2"], rec["u1"]:rec["u2"]]
    return float(np.abs(np.linalg.norm(_gaussian(c, rec["sigma_ran"]), axis=2) - 0.3).min())


INTS = ("v_ref", "u_ref", "v1", "v2", "u1", "u2", "shift_v", "shift_u", "shift_v_max", "shift_u_max", "side", "frame_h", "frame_w")


def load_samples(golden_dir):
    """The recorded get_patch_pair cases of tests/golden/reference_train_batch*.npz (make_reference_train_batch_vectors.py):
    a list of dicts -- name, patch, back, seed, batch_count, imsize, draws (list of float), ints (dict over INTS), angle, and the
    real function's src / tgt / mask as float64."""
    import os
    g = np.load(os.path.join(golden_dir, "reference_train_batch.npz"))
    assert str(g["version"]) == "0.18.3"
    outs = {}
    for i in range(int(g["n_parts"])):
        outs.update(np.load(os.path.join(golden_dir, "reference_train_batch_out%d.npz" % i)))
    scale = float(g["scale"])
    samples = []
    for k, name in enumerate(g["names"]):
        samples.append({"name": str(name), "patch": g["patch_%d" % k], "back": g["back_%d" % k], "seed": int(g["seed_%d" % k]),
                        "batch_count": int(g["batch_count_%d" % k]), "imsize": int(g["imsize_%d" % k]),
                        "draws": [float(v) for v in g["draws_%d" % k].view(np.float64)],
                        "ints": dict(zip(INTS, (int(v) for v in g["ints_%d" % k]))), "angle": float(g["angle_%d" % k].view(np.float64)),
                        "src": outs["src_%d" % k] / scale, "tgt": outs["tgt_%d" % k] / scale, "mask": outs["mask_%d" % k] / scale})
    return samples
