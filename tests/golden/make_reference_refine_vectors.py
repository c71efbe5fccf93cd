"""Golden vectors of the depth refinement from the REFERENCE'S OWN lines.

    python tests/golden/make_reference_refine_vectors.py <reference checkout>      (writes reference_refine.json)

pix2pose_util/common_util.py is imported as it stands (with np.float / np.int restored for numpy 2).  From
tools/5_evaluation_bop_icp3d.py the function icp_refinement() is taken out of the script's syntax tree and run unmodified, with:
    cv2           a stub: inpaint() is the onion-peel stand-in of DESIGN.md section 8 (tests/normals_ref.py); ppf_match_3d_ICP(...)
                  .registerModelToScene() is the ICP restatement of DESIGN.md section 8.2 (tests/icp_ref.py) with the parameters the
                  function constructs it with, and returns its pose (the residual is 0: the reference only reads its own -1)
    render_obj    tests/depth_ref.render_depth (the rasteriser's restatement) at the pose the function passes
    gpu_rendering False; obj_models / obj_order_id name the synthetic box mesh
The scene points are the script's :372-374 and the target points :464.  What is recorded is the function's return value: tf (4 x 4,
metres) or the -1 of its two gates, so the fixture pins the composition tf = pose . [R | t_adjusted / 1000] and its mm / m units
(:91-93), which icp3d.py :466-467 turn into R = tf[:3, :3], t = tf[:3, 3] * 1000.  The fixture stores only data: the frame, camera,
mesh, jobs and the results (arrays as zlib-compressed little-endian bytes in base64).
"""
import ast
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)
import depth_ref as D  # noqa: E402
import icp_ref as I  # noqa: E402
import normals_ref as N  # noqa: E402
from make_reference_normals_vectors import f32_b64, u8_b64  # noqa: E402

H, W = 48, 64
K = np.array([[120.0, 0.0, 31.63], [0.0, 123.0, 23.41], [0.0, 0.0, 1.0]])
MESH = D.box_mesh((-60.0, -45.0, -30.0), (60.0, 45.0, 30.0), 4)
R_TRUE = D.rot(0, 25.0) @ D.rot(1, -35.0) @ D.rot(2, 10.0)
T_TRUE = np.array([12.0, -8.0, 520.0])


def make_image():
    """The box at (R_TRUE, T_TRUE) in front of a slanted wall, with sensor noise and zero pixels."""
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    wall = (0.9 + 0.004 * jj + 0.002 * ii).astype(np.float32)
    obj = D.render_depth(*MESH, K, R_TRUE, T_TRUE, H, W)
    rs = np.random.RandomState(11)
    d = np.where(obj > 0, obj + rs.normal(scale=0.0005, size=obj.shape), wall).astype(np.float32)
    d[rs.rand(H, W) < 0.04] = 0
    return d, obj > 0


def make_jobs(d, silhouette):
    valid = (np.nan_to_num(d) > 0.2) & (np.nan_to_num(d) < 2.2)
    grown = silhouette.copy()
    grown[1:] |= grown[:-1]; grown[:-1] |= grown[1:]; grown[:, 1:] |= grown[:, :-1]; grown[:, :-1] |= grown[:, 1:]
    sparse = np.zeros((H, W), bool)
    sparse[[20, 21, 22, 26, 26, 27], [24, 25, 27, 30, 31, 32]] = True        # extent >= 5 in both axes, 6 pixels
    thin = np.zeros((H, W), bool)
    thin[22:26, 10:50] = True                                                 # 4 rows: the bbox gate
    return [
        {"R": (D.rot(1, 3.0) @ R_TRUE).tolist(), "t": (T_TRUE + [4.0, -3.0, 8.0]).tolist(), "mask": silhouette & valid, "why": "ok"},
        {"R": (D.rot(0, -2.5) @ D.rot(2, 2.0) @ R_TRUE).tolist(), "t": (T_TRUE + [-6.0, 2.0, -5.0]).tolist(), "mask": grown & valid,
         "why": "ok, grown mask"},
        {"R": R_TRUE.tolist(), "t": [T_TRUE[0], T_TRUE[1], 299.5], "mask": silhouette & valid, "why": "t < 300 replaced"},
        {"R": (D.rot(1, -4.0) @ R_TRUE).tolist(), "t": (T_TRUE + [2.0, 5.0, 3.0]).tolist(), "mask": grown & valid,
         "why": "ok, other start"},
        {"R": R_TRUE.tolist(), "t": T_TRUE.tolist(), "mask": thin & valid, "why": "bbox gate"},
        {"R": R_TRUE.tolist(), "t": T_TRUE.tolist(), "mask": sparse & valid, "why": "count gate"},
    ]


def load_reference(REF):
    np.float = float
    np.int = int
    captured = {}
    cv2 = types.ModuleType("cv2")
    cv2.INPAINT_NS = 0

    def inpaint(src, mask, radius, flags):
        assert radius == 2 and flags == cv2.INPAINT_NS
        return N.inpaint(src)

    class ICP:
        def __init__(self, iterations, tolerence, rejectionScale, numLevels):
            self.prm = dict(max_iterations=iterations, tolerance=tolerence, rejection_scale=rejectionScale, num_levels=numLevels)
            captured["params"] = self.prm

        def registerModelToScene(self, src, dst):
            r = I.icp(np.asarray(src, np.float32), np.asarray(dst, np.float32), **self.prm)
            captured["icp"] = r
            return 0, 0.0, r["pose"]

    cv2.inpaint = inpaint
    cv2.ppf_match_3d_ICP = ICP
    sys.modules["cv2"] = cv2
    sys.path.insert(0, REF)
    import pix2pose_util.common_util as cu

    src = open(os.path.join(REF, "tools", "5_evaluation_bop_icp3d.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "icp_refinement"][0]
    ns = {"np": np, "cv2": cv2, "getXYZ": cu.getXYZ, "get_normal": cu.get_normal, "get_bbox_from_mask": cu.get_bbox_from_mask,
          "gpu_rendering": False, "obj_order_id": 0, "obj_models": [MESH]}

    def render_obj(obj_m, rot, tra, cam_K, ren):
        return None, D.render_depth(*obj_m, cam_K, rot, np.array(tra, np.float64) * 1000.0, H, W)

    ns["render_obj"] = render_obj
    exec(compile(ast.Module([fn], []), "icp_refinement", "exec"), ns)
    return cu, ns["icp_refinement"], captured


def main(ref):
    cu, icp_refinement, cap = load_reference(ref)
    d, sil = make_image()
    scene = np.zeros((H, W, 6), np.float32)                             # icp3d.py:372-374
    scene[:, :, :3] = cu.getXYZ(d, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2])
    scene[:, :, 3:] = cu.get_normal(d, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], refine=True)
    out_jobs = []
    for j in make_jobs(d, sil):
        cap.pop("icp", None)
        union = j["mask"]
        pts_tgt = scene[union]                                          # :464
        tf, residual = icp_refinement(pts_tgt, MESH, np.array(j["R"]), np.array(j["t"], np.float64), K, None, union)
        rec = {"R": j["R"], "t": j["t"], "why": j["why"], "union_mask": u8_b64(union), "status": int(residual)}
        if residual != -1:
            r = cap["icp"]
            rec.update({"tf": np.asarray(tf).tolist(), "icp_pose": r["pose"].tolist(), "iterations": r["iterations"],
                        "pairs": r["pairs"]})
        out_jobs.append(rec)
        print(j["why"], rec["status"], rec.get("iterations", [])[:2], rec.get("pairs", [])[:2])
    fx = {"H": H, "W": W, "K": K.tolist(), "params": cap["params"], "true_R": R_TRUE.tolist(), "true_t": T_TRUE.tolist(),
          "mesh_verts": MESH[0].tolist(), "mesh_tris": np.asarray(MESH[1]).tolist(), "image": f32_b64(d), "jobs": out_jobs}
    json.dump(fx, open(os.path.join(HERE, "reference_refine.json"), "w"))


if __name__ == "__main__":
    main(sys.argv[1])
