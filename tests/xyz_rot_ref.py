"""numpy restatement of skimage.transform.rotate(image, angle, resize=True, cval=...) of scikit-image 0.17 / 0.18 (order 1, mode
'constant', clip=True) and, on top of it and of xyz_ref, of the in-plane rotation copies of the reference's
tools/2_2_render_pix2pose_training.py:64-96 (augment_inplane_gen, isYCB=False); for the tests only.  DESIGN.md section 8.4.

The rules, each held bit for bit to the real 0.18.3 by tests/test_xyz_rotate_cpu.py (tests/golden/skimage_rotate018.npz):

  * the matrix: tform1 = translation(centre), tform2 = rotation, tform3 = translation(-centre), tform = tform3 + tform2 + tform1,
    where a + b is b.params @ a.params, so tform.params = t1 @ (t2 @ t3) in that association; the output shape from the inverse
    image of the four corners; then translation((minc, minr)) + tform, i.e. tform.params @ t4, and the last row set to (0, 0, 1).
    The library does this with numpy's matmul and linalg.inv, whose last bit depends on the BLAS / LAPACK build underneath (numpy
    1.26 and 2.2 differ in the inverse); _mm and _inv3 write out the arithmetic of the build the fixture was recorded with;
  * a float64 image: every operation in double;
  * a float32 image: the matrix cast to float32; c = (M00 * x + M01 * y) + M02 and r likewise in float32 (the matrix of a rotation
    by k * 90 degrees has cos or sin of 6e-17, not 0, so it takes this path too); floorf / ceilf; dr = r - float(minr),
    dc = c - float(minc) in float32; then the interpolation is mixed: 1 - dc and 1 - dr are formed in DOUBLE, the left taps are
    multiplied in double, the right taps' products dc * top_right and dc * bottom_right are float32 products converted to double
    afterwards, top and bottom are double sums, (1 - dr) * top + double(dr) * bottom is double and rounded to float32 once;
  * the clip to the whole input's [min, max] (all channels), which keeps cval where cval lies outside that range.
"""
import math

import numpy as np

import xyz_ref as X

f32 = np.float32


def _mm(a, b):
    """a @ b in plain double products summed in index order, no fused multiply-add: what numpy's matmul gave under the library for
    these 3-column operands, written out so that the bits do not depend on the BLAS underneath."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros((a.shape[0], b.shape[1]))
    for i in range(a.shape[0]):
        for j in range(b.shape[1]):
            s = float(a[i, 0]) * float(b[0, j])
            for k in range(1, a.shape[1]):
                s = s + float(a[i, k]) * float(b[k, j])
            out[i, j] = s
    return out


def _inv3(m):
    """np.linalg.inv of a 3 x 3 matrix as LAPACK's dgesv computes it (held bit for bit to numpy 1.26 / OpenBLAS on the matrices of
    rotate): LU with partial pivoting, the column below a pivot scaled by the pivot's reciprocal, plain multiply-subtract updates,
    then per column of the identity the forward substitution and a back substitution that multiplies by the diagonal's reciprocal."""
    n = 3
    A = [[float(m[i][j]) for j in range(n)] for i in range(n)]
    B = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    for k in range(n):
        p = max(range(k, n), key=lambda i: (abs(A[i][k]), -i))
        if p != k:
            A[k], A[p] = A[p], A[k]
            B[k], B[p] = B[p], B[k]
        r = 1.0 / A[k][k]
        for i in range(k + 1, n):
            A[i][k] = A[i][k] * r
        for i in range(k + 1, n):
            for j in range(k + 1, n):
                A[i][j] = A[i][j] - A[i][k] * A[k][j]
    for c in range(n):
        for k in range(n):
            for i in range(k + 1, n):
                B[i][c] = B[i][c] - A[i][k] * B[k][c]
        for k in range(n - 1, -1, -1):
            B[k][c] = B[k][c] * (1.0 / A[k][k])
            for i in range(k):
                B[i][c] = B[i][c] - A[i][k] * B[k][c]
    return np.array(B)


def _translation(tx, ty):
    m = np.array([[1.0, -0.0, 0], [0.0, 1.0, 0], [0, 0, 1]])          # cos 0, -sin 0, sin 0 as the library's constructor leaves them
    m[0:2, 2] = (tx, ty)
    return m


def _rotation(a):
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])


def rotate_matrix(rows, cols, angle):
    """-> (float64 [3,3] map from output (x, y, 1) to input (c, r, 1), (out_rows, out_cols))."""
    center = np.array((cols, rows)) / 2. - 0.5
    t1, t2, t3 = _translation(*center), _rotation(np.deg2rad(angle)), _translation(*(-center))
    m = _mm(t1, _mm(t2, t3))
    corners = np.array([[0, 0], [0, rows - 1], [cols - 1, rows - 1], [cols - 1, 0]])
    x, y = np.transpose(corners)
    dst = _mm(np.vstack((x, y, np.ones_like(x))).T, _inv3(m).T)
    dst[dst[:, 2] == 0, 2] = np.finfo(float).eps
    dst[:, :2] /= dst[:, 2:3]
    minc, minr, maxc, maxr = dst[:, 0].min(), dst[:, 1].min(), dst[:, 0].max(), dst[:, 1].max()
    shape = np.around((maxr - minr + 1, maxc - minc + 1)).astype(int)
    m = _mm(m, _translation(minc, minr))
    m[2] = (0, 0, 1)
    return m, (int(shape[0]), int(shape[1]))


def _taps(img, minr, minc, maxr, maxc, cval):
    rows, cols = img.shape

    def px(rr, cc):
        ok = (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
        return np.where(ok, img[np.clip(rr, 0, rows - 1), np.clip(cc, 0, cols - 1)], img.dtype.type(cval))
    return px(minr, minc), px(minr, maxc), px(maxr, minc), px(maxr, maxc)


def warp_f64(img, m, shape, cval):
    """One float64 channel [rows, cols] -> float64 [shape], unclipped."""
    y, x = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    c = m[0, 0] * x + m[0, 1] * y + m[0, 2]
    r = m[1, 0] * x + m[1, 1] * y + m[1, 2]
    minr, minc, maxr, maxc = (np.floor(r).astype(np.int64), np.floor(c).astype(np.int64), np.ceil(r).astype(np.int64),
                              np.ceil(c).astype(np.int64))
    dr, dc = r - minr, c - minc
    tl, tr, bl, br = _taps(img, minr, minc, maxr, maxc, cval)
    top = (1 - dc) * tl + dc * tr
    bottom = (1 - dc) * bl + dc * br
    return (1 - dr) * top + dr * bottom


def warp_f32(img, m, shape, cval):
    """One float32 channel [rows, cols] -> float32 [shape], unclipped; m is the float64 matrix (cast here)."""
    assert img.dtype == np.float32
    m = np.asarray(m).astype(f32)
    y, x = np.meshgrid(np.arange(shape[0], dtype=f32), np.arange(shape[1], dtype=f32), indexing="ij")
    c = (m[0, 0] * x + m[0, 1] * y) + m[0, 2]
    r = (m[1, 0] * x + m[1, 1] * y) + m[1, 2]
    assert c.dtype == np.float32 and r.dtype == np.float32
    fr, fc = np.floor(r), np.floor(c)
    minr, minc, maxr, maxc = fr.astype(np.int64), fc.astype(np.int64), np.ceil(r).astype(np.int64), np.ceil(c).astype(np.int64)
    dr, dc = r - fr, c - fc                                            # float32 - float32(long)
    tl, tr, bl, br = _taps(img, minr, minc, maxr, maxc, f32(cval))
    one_dc, one_dr = 1.0 - dc.astype(np.float64), 1.0 - dr.astype(np.float64)
    top = one_dc * tl.astype(np.float64) + (dc * tr).astype(np.float64)
    bottom = one_dc * bl.astype(np.float64) + (dc * br).astype(np.float64)
    return (one_dr * top + dr.astype(np.float64) * bottom).astype(f32)


def clip_warp(inp, out, cval):
    """_clip_warp_output: in place on out."""
    lo, hi = inp.min(), inp.max()
    keep = out == cval if not (lo <= cval <= hi) else None
    np.clip(out, lo, hi, out=out)
    if keep is not None:
        out[keep] = cval
    return out


def rotate(img, angle, cval=0.0):
    """rotate(img, angle, resize=True, cval=cval) for a float32 or float64 image [rows, cols] or [rows, cols, ch]."""
    img = np.asarray(img)
    assert img.dtype in (np.float32, np.float64)
    m, shape = rotate_matrix(img.shape[0], img.shape[1], angle)
    warp = warp_f32 if img.dtype == np.float32 else warp_f64
    if img.ndim == 2:
        out = warp(img, m, shape, cval)
    else:
        out = np.dstack([warp(np.ascontiguousarray(img[..., k]), m, shape, cval) for k in range(img.shape[2])])
    return clip_warp(img, out, cval)


def input_tables():
    """The two float32 images augment_inplane_gen rotates, as 256-entry tables of the 8-bit value they come from.
    rgb: (img / 255).astype(float32) of the uint8 frame (a double division).  xyz: img_r is the read-back float32(q) / 255 times 255
    in float32 (get_rendering), and (img_r / 255) divides that float32 array again: float32(float32(float32(q) / 255) * 255) / 255."""
    q = np.arange(256)
    rgb = (q.astype(np.uint8) / 255).astype(f32)
    qf = q.astype(f32)
    xyz = ((qf / f32(255)) * f32(255)) / f32(255)
    assert xyz.dtype == np.float32
    return rgb, xyz


def levels(color):
    """float colour in [0, 1] -> the GL buffer's 8-bit level q (xyz_ref.quantise without its table)."""
    return np.clip(np.floor(np.asarray(color, np.float64) * 255 + 0.5).astype(np.int64), 0, 255)


def box_of_mask(depth_rot):
    """2_2:74-75 -> [min v, min u, max v, max u] of depth_rot > 0 (max inclusive), or None when nothing is."""
    vv, uu = np.nonzero(depth_rot > 0)
    if len(vv) == 0:
        return None
    return [int(vv.min()), int(uu.min()), int(vv.max()), int(uu.max())]


def crop_patch(img_rot, img_r_rot, box):
    """2_2:76-80: the uint8 [h, w, 6] patch of the two rotated images times 255 (float32), truncated; the slice leaves the box's last
    row and column out.  None for a zero side."""
    h, w = box[2] - box[0], box[3] - box[1]
    if h == 0 or w == 0:
        return None
    data = np.zeros((h, w, 6), np.uint8)
    data[:, :, :3] = (img_rot * 255)[box[0]:box[2], box[1]:box[3]]
    data[:, :, 3:6] = (img_r_rot * 255)[box[0]:box[2], box[1]:box[3]]
    return data


def resize_patch(data, gen=1):
    """2_2:85-95: each half resized on its own when the longer side exceeds 128 (xyz_ref.patch's rule)."""
    from oracle import est_pose_oracle as O
    oh, ow = X.patch_shape(*data.shape[:2])
    if (oh, ow) == data.shape[:2]:
        return data
    if oh == 0 or ow == 0:
        return None
    new = np.zeros((oh, ow, 6), np.uint8)
    mode = "constant" if gen == 0 else "reflect"
    for s in (slice(0, 3), slice(3, 6)):
        new[:, :, s] = (O.resize_gen((data[:, :, s] / 255).astype(f32), (oh, ow), mode, 0.0, gen) * 255).astype(np.uint8)
    return new


def rotated_unresized(rgb_u8, color, depth, angle):
    """One angle of augment_inplane_gen up to the crop.  rgb_u8: the frame as loaded; color, depth: the render."""
    rgb_tab, xyz_tab = input_tables()
    img = np.array(rgb_u8, np.uint8)
    img[np.asarray(depth) == 0] = [128, 128, 128]
    img_r_rot = rotate(xyz_tab[levels(color)], angle, cval=0)
    img_rot = rotate(rgb_tab[img], angle, cval=0.5)
    depth_rot = rotate((np.asarray(depth) > 0).astype(np.float64), angle)
    box = box_of_mask(depth_rot)
    if box is None:
        return None
    return crop_patch(img_rot, img_r_rot, box)


def augment_inplane(rgb_u8, color, depth, angles, gen=1):
    """-> one uint8 [h, w, 6] patch (or None) per angle; gen: the resize generation of boxes above 128 px (1 = 0.17 / 0.18, the one
    whose rotate this file restates)."""
    out = []
    for a in angles:
        data = rotated_unresized(rgb_u8, color, depth, a)
        out.append(None if data is None else resize_patch(data, gen))
    return out
