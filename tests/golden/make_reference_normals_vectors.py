"""Golden vectors of depth back-projection, normals and the ICP point sets from the REFERENCE'S OWN lines.

    python tests/golden/make_reference_normals_vectors.py <reference checkout>      (writes reference_normals.json)

pix2pose_util/common_util.py is imported as it stands (with np.float / np.int restored for numpy 2).  From
tools/5_evaluation_bop_icp3d.py the function icp_refinement() is taken out of the script's syntax tree and run unmodified, with:
    cv2           a stub: inpaint() is the onion-peel stand-in of DESIGN.md section 8 (tests/normals_ref.py), ppf_match_3d_ICP(...)
                  .registerModelToScene() records the two point arrays it is handed and returns an identity pose
    render_obj    tests/depth_ref.render_depth (the rasteriser's restatement) at the pose the function passes
    gpu_rendering False; obj_models / obj_order_id name the synthetic box mesh
The scene points are the script's :372-374 (getXYZ and get_normal(refine=True) into a float32 [H, W, 6]) and the target points
:464 (points_tgt[union_mask]; stored as its count: the points are scene_points[union_mask]).  The fixture stores only data:
the frame, camera, jobs and what the reference computed (arrays as zlib-compressed little-endian bytes in base64).
"""
import ast
import base64
import json
import os
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import depth_ref as D  # noqa: E402
import normals_ref as N  # noqa: E402

H, W = 24, 32
K = np.array([[60.0, 0.0, 15.63], [0.0, 61.5, 11.41], [0.0, 0.0, 1.0]])
MESH = D.box_mesh((-60.0, -45.0, -30.0), (60.0, 45.0, 30.0), 4)


def f32_b64(a):
    return base64.b64encode(zlib.compress(np.ascontiguousarray(a, "<f4").tobytes(), 9)).decode()


def b64_f32(s, shape):
    return np.frombuffer(zlib.decompress(base64.b64decode(s)), "<f4").reshape(shape).copy()


def u8_b64(a):
    return base64.b64encode(zlib.compress(np.ascontiguousarray(a, np.uint8).tobytes(), 9)).decode()


def b64_u8(s, shape):
    return np.frombuffer(zlib.decompress(base64.b64decode(s)), np.uint8).reshape(shape).copy()


R0 = D.rot(0, 25.0) @ D.rot(1, -35.0) @ D.rot(2, 10.0)
T0 = np.array([12.0, -8.0, 520.0])


def make_images():
    """One sensor frame: the box at (R0, T0) in front of a slanted wall, with zero and NaN pixels, a NaN block, and a hole in the
    top-left corner whose corner pixels are more than FILL_LAYERS px from any known pixel."""
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    wall = (0.9 + 0.004 * jj + 0.002 * ii).astype(np.float32)
    obj = D.render_depth(*MESH, K, R0, T0, H, W)
    d = np.where(obj > 0, obj, wall).astype(np.float32)
    rs = np.random.RandomState(5)
    d[rs.rand(H, W) < 0.04] = 0
    d[rs.rand(H, W) < 0.02] = np.nan
    d[0:13, 0:13] = 0
    d[1:4, 24:30] = np.nan
    return [d]


def make_jobs(images):
    valid = [np.nan_to_num(d) > 0.2 for d in images]
    valid = [v & (np.nan_to_num(d) < 2.2) for v, d in zip(valid, images)]

    def rect(r0, c0, r1, c1):
        m = np.zeros((H, W), bool)
        m[r0:r1, c0:c1] = True
        return m

    sparse = np.zeros((H, W), bool)
    sparse[[8, 9, 10, 14, 14, 15], [12, 13, 15, 18, 19, 20]] = True       # extent >= 5 in both axes, 6 pixels
    v = valid[0]
    return [
        {"image": 0, "t": (T0 + [3.0, -2.0, 6.0]).tolist(), "mask": rect(1, 3, 23, 30) & v, "why": "ok"},
        {"image": 0, "t": [T0[0], T0[1], 299.5], "mask": rect(3, 6, 21, 28) & v, "why": "t < 300 replaced"},
        {"image": 0, "t": [T0[0], T0[1], 5000.5], "mask": rect(3, 6, 21, 28) & v, "why": "t > 5000 replaced"},
        {"image": 0, "t": T0.tolist(), "mask": rect(10, 8, 14, 24) & v, "why": "bbox gate (4 rows)"},
        {"image": 0, "t": T0.tolist(), "mask": sparse & v, "why": "count gate"},
        {"image": 0, "t": (T0 + [0.0, 0.0, 4.0]).tolist(), "mask": rect(0, 0, H, W) & v, "why": "whole-frame union"},
    ]


def load_reference(REF):
    np.float = float
    np.int = int
    captured = {}
    cv2 = types.ModuleType("cv2")
    cv2.INPAINT_NS = 0

    def inpaint(src, mask, radius, flags):
        assert radius == 2 and flags == cv2.INPAINT_NS
        assert np.array_equal(mask != 0, np.nan_to_num(src) == 0)
        return N.inpaint(src)

    class ICP:
        def __init__(self, *a, **k):
            pass

        def registerModelToScene(self, src, dst):
            captured["src"], captured["tgt"] = np.array(src, np.float32), np.array(dst, np.float32)
            return 0, 0.0, np.eye(4)

    cv2.inpaint = inpaint
    cv2.ppf_match_3d_ICP = ICP
    sys.modules["cv2"] = cv2
    sys.path.insert(0, REF)
    import pix2pose_util.common_util as cu

    src = open(os.path.join(REF, "tools", "5_evaluation_bop_icp3d.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "icp_refinement"][0]
    ns = {"np": np, "cv2": cv2, "getXYZ": cu.getXYZ, "get_normal": cu.get_normal, "gpu_rendering": False, "obj_order_id": 0,
          "obj_models": [MESH]}

    def bbox_rec(mask):
        captured["bbox"] = cu.get_bbox_from_mask(mask)
        return captured["bbox"]

    def render_obj(obj_m, rot, tra, cam_K, ren):
        captured["t_init"] = np.array(tra, np.float64) * 1000.0
        return None, D.render_depth(*obj_m, cam_K, rot, captured["t_init"], H, W)

    ns["get_bbox_from_mask"] = bbox_rec
    ns["render_obj"] = render_obj
    exec(compile(ast.Module([fn], []), "icp_refinement", "exec"), ns)
    return cu, ns["icp_refinement"], captured


def main(ref):
    cu, icp_refinement, cap = load_reference(ref)
    images = make_images()
    scene = []
    for d in images:
        pts = np.zeros((H, W, 6), np.float32)                        # icp3d.py:372-374
        pts[:, :, :3] = cu.getXYZ(d, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2])
        pts[:, :, 3:] = cu.get_normal(d, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], refine=True)
        scene.append(pts)
    out_jobs = []
    for j in make_jobs(images):
        cap.clear()
        union = j["mask"]
        pts_tgt = scene[j["image"]][union]                            # :464
        tf, residual = icp_refinement(pts_tgt, MESH, R0, np.array(j["t"], np.float64), K, None, union)
        rec = {"image": j["image"], "t": j["t"], "why": j["why"], "union_mask": u8_b64(union), "status": int(residual),
               "bbox": [int(x) for x in cap["bbox"]], "t_init": cap["t_init"].tolist(), "n_tgt": int(len(pts_tgt))}
        if residual != -1:
            rec.update({"t_adjusted": (tf[:3, 3] * 1000.0).tolist(), "n_src": int(len(cap["src"])), "src": f32_b64(cap["src"])})
            assert np.array_equal(cap["tgt"], pts_tgt)
        out_jobs.append(rec)
        print(j["why"], rec["status"], rec["bbox"], rec.get("n_src"), rec["n_tgt"])
    fx = {"H": H, "W": W, "K": K.tolist(), "R": R0.tolist(), "mesh_verts": MESH[0].tolist(), "mesh_tris": np.asarray(MESH[1]).tolist(),
          "images": [f32_b64(d) for d in images], "scene_points": [f32_b64(p) for p in scene], "jobs": out_jobs}
    json.dump(fx, open(os.path.join(HERE, "reference_normals.json"), "w"))


if __name__ == "__main__":
    main(sys.argv[1])
