"""XYZ-coloured object models: the host side of the training-target renders.

Restates the reference's tools/2_1_ply_file_to_3d_coord_model.py (convert_unique with all three axes centred: every vertex is
coloured by its normalised object coordinate) and get_sympose of tools/2_2_render_pix2pose_training.py:26-52 (the rotation about a
continuous symmetry axis is taken out of a ground-truth pose before it is rendered).  The colour rasteriser itself is
csrc/depth.hip (runtime.render_xyz_batch).
"""
from __future__ import annotations

import json
import os

import numpy as np

from .mesh import read_ply, read_ply_rgb, write_ply_rgb

NORM_KEYS = ("x_scale", "y_scale", "z_scale", "x_ct", "y_ct", "z_ct")


def xyz_colors(verts_mm):
    """convert_unique (2_1:30-63), all axes centred -> (colors uint8 [N,3], norm_factor dict).

    Per axis: ct = mean, abs = max|x - ct|, c = ((x - ct) / abs + 1) / 2 * 255, all in float32 -- plyfile holds the vertex
    properties as float32 and numpy's mean of a float32 array is a float32 -- and the value is stored into a uchar property, which
    truncates toward zero.  norm_factor holds x_scale .. z_ct as Python floats (what 2_1 writes to norm_factor.json)."""
    v = np.ascontiguousarray(verts_mm, dtype=np.float32).reshape(-1, 3)
    colors = np.empty(v.shape, np.uint8)
    norm = {}
    for k, ax in enumerate("xyz"):
        x = v[:, k]
        ct = np.mean(x)                                  # float32
        ab = np.max(np.abs(x - ct))
        if not ab > 0:
            raise ValueError("xyz_colors: the mesh is flat along %s (max|%s - mean| = %r): no coordinate to encode" % (ax, ax, float(ab)))
        c = ((x - ct) / ab + np.float32(1)) / np.float32(2) * np.float32(255)
        colors[:, k] = c.astype(np.uint8)
        norm[ax + "_scale"] = float(ab)
        norm[ax + "_ct"] = float(ct)
    return colors, norm


def write_models_xyz(models_dir, out_dir, obj_ids=None):
    """Step 2_1 for a BOP models directory: every models_dir/obj_<id:06d>.ply (or those of obj_ids) is written to
    out_dir/obj_<id:06d>.ply with its XYZ colours, and out_dir/norm_factor.json gets {obj_id: norm_factor}.  -> that dict."""
    if obj_ids is None:
        obj_ids = sorted(int(f[4:-4]) for f in os.listdir(models_dir) if f.startswith("obj_") and f.endswith(".ply"))
    os.makedirs(out_dir, exist_ok=True)
    param = {}
    for oid in obj_ids:
        name = "obj_%06d.ply" % int(oid)
        verts, tris = read_ply(os.path.join(models_dir, name))
        colors, norm = xyz_colors(verts)
        write_ply_rgb(os.path.join(out_dir, name), verts, tris, colors)
        param[int(oid)] = norm
    write_norm_factor(os.path.join(out_dir, "norm_factor.json"), param)
    return param


def write_norm_factor(path, param):
    with open(path, "w") as f:
        json.dump({str(k): {n: float(v[n]) for n in NORM_KEYS} for k, v in param.items()}, f, indent=2, sort_keys=True)


def read_norm_factor(path):
    """-> {int obj_id: {x_scale, y_scale, z_scale, x_ct, y_ct, z_ct}}"""
    with open(path) as f:
        return {int(k): {n: float(v[n]) for n in NORM_KEYS} for k, v in json.load(f).items()}


def read_xyz_model(path):
    """A models_xyz PLY -> (verts mm, tris, colors uint8 [N,3]); a file without vertex colours is an error."""
    verts, tris, colors = read_ply_rgb(path)
    if colors is None:
        raise ValueError("%s has no red / green / blue vertex properties" % path)
    return verts, tris, colors


# ---- static-frame Euler angles of three distinct axes -------------------------------------------------------------------
# Order "s" + a1 a2 a3 means: rotate about the fixed axis a1 by the first angle, then about the fixed a2, then about the fixed a3,
# so R = R_a3(third) @ R_a2(second) @ R_a1(first).  get_sympose can form xyz, yxz, zxy (one symmetry axis) and xzy, yzx (two axes
# flagged); any permutation works here.

def _axis_rot(ax, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][ax]
    R = np.eye(3)
    R[i, i] = c; R[j, j] = c; R[i, j] = -s; R[j, i] = s
    return R


def euler2mat_static(a1, a2, a3, order):
    i, j, k = ("xyz".index(c) for c in order)
    return _axis_rot(k, a3) @ _axis_rot(j, a2) @ _axis_rot(i, a1)


def mat2euler_static(R, order):
    """Inverse of euler2mat_static for three distinct axes.  With i, j, k the axes in order and sg = +1 for an even permutation
    of xyz, -1 for an odd one: R[k,i] = -sg sin(a2), R[i,i] = cos a2 cos a3, R[j,i] = sg cos a2 sin a3, R[k,j] = sg sin a1 cos a2,
    R[k,k] = cos a1 cos a2.  At the gimbal lock (cos a2 = 0) the third angle is set to 0 and the first takes the whole turn."""
    M = np.asarray(R, np.float64).reshape(3, 3)
    i, j, k = ("xyz".index(c) for c in order)
    if sorted((i, j, k)) != [0, 1, 2]:
        raise ValueError("axis order %r does not name three distinct axes" % (order,))
    sg = 1.0 if (j - i) % 3 == 1 else -1.0
    cy = np.hypot(M[i, i], M[j, i])
    if cy > 4 * np.finfo(np.float64).eps:
        a1 = np.arctan2(sg * M[k, j], M[k, k])
        a2 = np.arctan2(-sg * M[k, i], cy)
        a3 = np.arctan2(sg * M[j, i], M[i, i])
    else:
        a1 = np.arctan2(-sg * M[j, k], M[j, j])
        a2 = np.arctan2(-sg * M[k, i], cy)
        a3 = 0.0
    return a1, a2, a3


def get_sympose(R, sym):
    """get_sympose (2_2:26-52): -> (R', rotation_lock).  sym is the six numbers 2_2 builds (axis of the first continuous
    symmetry, then its offset; all zero without one); only sym[:3] is used.

    When sum(sym) > 0 the static-frame Euler order lists the axes flagged sym[a] == 1 first, then the others; the pose is
    decomposed in that order, the angles about the flagged axes are zeroed and the matrix is recomposed -- so R = R' @ (a
    rotation about the symmetry axis), and every pose of a symmetric object that looks the same renders the same target.
    rotation_lock is True when the recomposed pose carries the symmetry axis within |axis . z| > 0.8 of the camera axis: the
    reference then skips its in-plane rotation copies, and so does make_train_xyz.  Without a symmetry R is returned unchanged."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    sym = np.asarray(sym, np.float64).ravel()
    if not np.sum(sym) > 0:
        return R, False
    flagged = [a for a in range(3) if sym[a] == 1]
    others = [a for a in range(3) if sym[a] == 0]
    order = "".join("xyz"[a] for a in flagged + others)
    if len(order) != 3:
        raise ValueError("symmetry axis %r: every component must be 0 or 1" % (sym[:3].tolist(),))
    ang = list(mat2euler_static(R, order))
    for n in range(len(flagged)):
        ang[n] = 0.0
    Rn = euler2mat_static(ang[0], ang[1], ang[2], order)
    lock = bool(abs(float((Rn @ sym[:3])[2])) > 0.8)
    return Rn, lock
