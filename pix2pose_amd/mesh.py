"""BOP object meshes: a numpy-only PLY reader (``models/obj_<id:06d>.ply``).

The reference loads these through plyfile (rendering/model.py Model3D.load, bop_toolkit inout.load_ply) and keeps
vertex ``x y z`` (mm) and ``face vertex_indices``; this reader does the same for ``ascii`` and ``binary_little_endian``
files.  Polygons are fan-triangulated ((0,1,2), (0,2,3), ...); every other element and property is read past and dropped.
"""
from __future__ import annotations

import numpy as np

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}
_FACE_LISTS = ("vertex_indices", "vertex_index")
_RGB = ("red", "green", "blue")


def _parse_header(f):
    if f.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError("PLY header has no end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError("PLY property before any element")
            if tok[1] == "list":
                elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
        elif tok[0] == "end_header":
            break
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("unsupported PLY format %r" % (fmt,))
    return fmt, elements


def _fan(polys):
    tris = []
    for p in polys:
        for k in range(1, len(p) - 1):
            tris.append((p[0], p[k], p[k + 1]))
    return tris


def _read_ascii(f, elements, rgb=None):
    tokens = f.read().split()
    pos = 0
    out = {}
    for name, count, props in elements:
        rows = []
        for _ in range(count):
            row = {}
            for pname, t, it in props:
                if it is None:
                    row[pname] = float(tokens[pos]) if t[0] == "f" else int(tokens[pos])
                    pos += 1
                else:
                    n = int(tokens[pos])
                    row[pname] = [int(x) for x in tokens[pos + 1:pos + 1 + n]]
                    pos += 1 + n
            rows.append(row)
        out[name] = rows
    verts = np.array([[r["x"], r["y"], r["z"]] for r in out.get("vertex", [])], np.float64).reshape(-1, 3)
    names = {p[0] for e in elements if e[0] == "vertex" for p in e[2]}
    if rgb is not None and all(c in names for c in _RGB):
        rgb.append(np.array([[r[c] for c in _RGB] for r in out.get("vertex", [])], np.uint8).reshape(-1, 3))
    key = next((p[0] for e in elements if e[0] == "face" for p in e[2] if p[0] in _FACE_LISTS), None)
    polys = [r[key] for r in out.get("face", [])] if key else []
    return verts, polys


def _read_binary(buf, elements, rgb=None):
    pos = 0
    verts, polys = np.zeros((0, 3)), []
    for name, count, props in elements:
        if all(it is None for _, _, it in props):
            dt = np.dtype([(p, "<" + t) for p, t, _ in props])
            arr = np.frombuffer(buf, dt, count, pos)
            pos += dt.itemsize * count
            if name == "vertex":
                verts = np.stack([arr["x"], arr["y"], arr["z"]], 1).astype(np.float64)
                if rgb is not None and all(c in dt.names for c in _RGB):
                    rgb.append(np.stack([arr[c] for c in _RGB], 1).astype(np.uint8))
            continue
        if len(props) == 1 and count > 0:
            # fast path: every polygon has as many corners as the first (BOP models are all triangles)
            _, t, it = props[0]
            n0 = int(np.frombuffer(buf, "<" + t, 1, pos)[0])
            dt = np.dtype([("n", "<" + t), ("v", "<" + it, (n0,))])
            if pos + dt.itemsize * count <= len(buf):
                arr = np.frombuffer(buf, dt, count, pos)
                if np.all(arr["n"] == n0):
                    pos += dt.itemsize * count
                    if name == "face" and props[0][0] in _FACE_LISTS:
                        polys = arr["v"].astype(np.int64).tolist()
                    continue
        rows = []
        for _ in range(count):
            row = None
            for pname, t, it in props:
                if it is None:
                    pos += np.dtype(t).itemsize
                    continue
                n = int(np.frombuffer(buf, "<" + t, 1, pos)[0])
                pos += np.dtype(t).itemsize
                vals = np.frombuffer(buf, "<" + it, n, pos)
                pos += np.dtype(it).itemsize * n
                if name == "face" and pname in _FACE_LISTS:
                    row = [int(x) for x in vals]
            if row is not None:
                rows.append(row)
        if name == "face":
            polys = rows
    return verts, polys


def _read(path, rgb):
    with open(path, "rb") as f:
        fmt, elements = _parse_header(f)
        if fmt == "ascii":
            verts, polys = _read_ascii(f, elements, rgb)
        else:
            verts, polys = _read_binary(f.read(), elements, rgb)
    tris = np.array(_fan(polys), np.int32).reshape(-1, 3)
    if tris.size and (tris.min() < 0 or tris.max() >= len(verts)):
        raise ValueError("%s: a face names a vertex outside [0, %d)" % (path, len(verts)))
    return verts, tris


def read_ply(path):
    """-> (verts float64 [N,3] in the file's units (mm for BOP models), tris int32 [M,3]) with polygons fan-triangulated."""
    return _read(path, None)


def read_ply_rgb(path):
    """read_ply plus the vertex colours: -> (verts, tris, colors uint8 [N,3] = the vertex element's red, green, blue, or None when
    it does not have all three)."""
    rgb = []
    verts, tris = _read(path, rgb)
    return verts, tris, (rgb[0] if rgb else None)


def write_ply_rgb(path, verts, tris, colors):
    """A binary_little_endian PLY with float x y z, uchar red green blue and triangle faces (what a models_xyz file needs)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    c = np.asarray(colors, np.uint8).reshape(-1, 3)
    t = np.asarray(tris, np.int32).reshape(-1, 3)
    if len(c) != len(v):
        raise ValueError("%d colours for %d vertices" % (len(c), len(v)))
    va = np.empty(len(v), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    for k, n in enumerate("xyz"):
        va[n] = v[:, k]
    for k, n in enumerate(_RGB):
        va[n] = c[:, k]
    fa = np.empty(len(t), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    fa["n"] = 3
    fa["v"] = t
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(v), len(t)))
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(va.tobytes())
        f.write(fa.tobytes())
