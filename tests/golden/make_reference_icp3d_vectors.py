"""Golden vectors of the RGB-D evaluation loop from the REFERENCE'S OWN lines.

    python tests/golden/make_reference_icp3d_vectors.py <reference checkout>      (writes reference_icp3d.json)

From tools/5_evaluation_bop_icp3d.py the function fcn(), the per-image loop ``for scene_id, im_id, obj_id_targets, inst_counts in
target_list:`` and the result-writing lines after it are taken out of the script's syntax tree and run unmodified, with stubs:
    inout                 load_scene_camera / load_im / load_depth over the small arrays below; save_bop_results records its rows
    get_rcnn_detection    scripted rois, obj ids, scores and masks [H, W, n] of the current image
    obj_pix2pose[k]       est_pose() returns the scripted outcome of (roi, object) -- frac_inlier -1, a t_z below 0.2 m, or a pose --
                          and logs the call
    icp_refinement        the scripted tf (4 x 4, metres) or -1, and logs the call with its union size
    render_obj            a depth equal to depth_t at the scripted inlier pixels of the union and 0.5 m off elsewhere, so that fcn is
                          the inlier count exactly and ratio an exact ratio of counts
    getXYZ / get_normal   zeros (only the stubbed icp_refinement would read them)
    np.int / np.float restored for numpy 2; dummy_run = False, gpu_rendering = False, task_type 2.
Detector scores are float64, as the dump hands them to the driver (JSON numbers), and the rendered depth is float64, so fcn is a
float64 exact integer and every score a float64 product under numpy 1 and 2 alike (with a float32 fcn, numpy 2 would keep the round-1
score 0.001 * fcn in float32).
Recorded: result_dataset, and per image the est_pose and ICP call logs.  The fixture holds data only: the depth frame, the detector
masks, the outcome tables with their rendered depths (zlib-compressed little-endian arrays in base64) and the results.

Scenario (one image each unless said): A -- an obj-1 roi skipped by the bool occupancy, the same situation for obj 2 not skipped, a
NaN IoU (empty mask), a (-1, -1) roi, unions of 30 and 31 pixels, est_pose -1, t_z < 0.2 m, ICP -1; B -- a round-1 roi with two
candidates whose last scored one is not the best (its mask decides the next roi's skip), the missing set shrinking mid-round and the
round-1 break; C -- best_ratio exactly 0.5 and just above, an IoU of exactly 7/10; D -- ViVo truncation; E -- an image with no result.
"""
import ast
import io
import json
import os
import sys
import types
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_normals_vectors import f32_b64, u8_b64  # noqa: E402

H, W = 32, 40
K = np.array([[60.0, 0.0, 19.5], [0.0, 61.0, 15.5], [0.0, 0.0, 1.0]])
MODEL_IDS = [1, 2, 3, 4, 5, 6, 7]


def rect(r0, r1, c0, c1):
    m = np.zeros((H, W), bool)
    m[r0:r1, c0:c1] = True
    return m


def raw_depth():
    d = np.full((H, W), 1000.0, np.float32)        # 1 m at depth_scale 1.0
    d[31, :] = 0                                  # a row of holes: not valid, never in a union
    d[0, 0] = np.nan
    return d


def first_k(mask, k, last=False):
    idx = np.flatnonzero(mask.reshape(-1))
    sel = idx[-k:] if last else idx[:k]
    out = np.zeros(H * W, bool)
    if k > 0:
        out[sel] = True
    return out.reshape(H, W)


def ok(k, last=False, dz=0.0):
    R = np.eye(3)
    return {"est": "ok", "R_est": R.tolist(), "t_est": [10.0, -5.0, 800.0 + dz], "icp": "ok",
            "tf": [[1, 0, 0, 0.011], [0, 1, 0, -0.004], [0, 0, 1, 0.801 + dz / 1000], [0, 0, 0, 1]], "k": k, "last": last}


EST_FAIL = {"est": "fail"}
NEAR = {"est": "ok", "R_est": np.eye(3).tolist(), "t_est": [0.0, 0.0, 150.0], "icp": "ok"}
ICP_FAIL = {"est": "ok", "R_est": np.eye(3).tolist(), "t_est": [0.0, 0.0, 700.0], "icp": "fail"}


def scenario():
    """-> list of images: scene_id, im_id, targets, counts, rois, obj_ids, scores, masks, outcomes {(r_id, obj_id): outcome}."""
    ims = []
    box = [4, 4, 10, 10]
    # A
    M1, M2 = rect(2, 8, 2, 8), rect(12, 22, 2, 12)        # |M2| / |M1 u M2| = 100 / 136 > 0.7: "occupancy != 0" would skip roi 3
    m31 = rect(22, 27, 12, 18)
    m31[27, 12] = True
    masks = [M1, M1, M2, M2, np.zeros((H, W), bool), M2, rect(22, 27, 2, 8), m31, rect(2, 10, 20, 28), rect(12, 20, 20, 28),
             rect(22, 30, 20, 28)]
    obj = [1, 1, 2, 2, 2, 2, 2, 2, 1, 1, 1]
    rois = [[2 + r, 2, 10, 10] for r in range(len(masks))]
    rois[5] = [-1, -1, 5, 5]
    out = {(0, 1): ok(36), (1, 1): ok(10), (2, 2): ok(100), (3, 2): ok(40, last=True), (4, 2): ok(5), (5, 2): ok(5), (6, 2): ok(20),
           (7, 2): ok(20), (8, 1): EST_FAIL, (9, 1): NEAR, (10, 1): ICP_FAIL}
    ims.append({"scene_id": 1, "im_id": 1, "targets": [1, 2], "counts": [2, 3], "rois": rois, "obj_ids": obj,
                "scores": [0.9, 0.8, 0.7, 0.6, 0.5, 0.5, 0.4, 0.3, 0.3, 0.2, 0.1], "masks": masks, "out": out})
    # B: round 1 only (non-target detections)
    P = rect(2, 12, 2, 12)
    X = first_k(P, 60, last=True)
    masks = [P, X, rect(14, 24, 2, 12), rect(14, 24, 20, 30)]
    out = {(0, 3): ok(80), (0, 4): ok(60, last=True), (1, 4): ok(60), (2, 4): ok(90), (3, 4): ok(90)}
    ims.append({"scene_id": 1, "im_id": 2, "targets": [3, 4], "counts": [1, 1], "rois": [box] * 4, "obj_ids": [9] * 4,
                "scores": [0.9] * 4, "masks": masks, "out": out})
    # C: ratio 0.5 (row, no update), 0.6 (update), an IoU of exactly 42/60 = 0.7 (not skipped), 0.51 (just above)
    Q, Q2 = rect(2, 12, 2, 12), rect(14, 24, 2, 12)
    D = first_k(Q2, 42)
    masks = [Q, Q2, D, rect(2, 12, 20, 30)]
    out = {(0, 5): ok(50), (1, 5): ok(60), (2, 5): ok(35), (3, 5): ok(51)}
    ims.append({"scene_id": 2, "im_id": 1, "targets": [5], "counts": [3], "rois": [box] * 4, "obj_ids": [9] * 4, "scores": [0.9] * 4,
                "masks": masks, "out": out})
    # D: two results for one instance (ViVo keeps the better one)
    masks = [rect(2, 12, 2, 12), rect(14, 24, 2, 12)]
    out = {(0, 6): ok(70), (1, 6): ok(90)}
    ims.append({"scene_id": 2, "im_id": 2, "targets": [6], "counts": [1], "rois": [box] * 2, "obj_ids": [6, 6], "scores": [0.9, 0.8],
                "masks": masks, "out": out})
    # E: no result
    ims.append({"scene_id": 3, "im_id": 1, "targets": [7], "counts": [1], "rois": [box], "obj_ids": [7], "scores": [0.9],
                "masks": [rect(2, 12, 2, 12)], "out": {(0, 7): EST_FAIL}})
    return ims


def run_reference(REF, ims):
    np.float = float
    np.int = int
    src = open(os.path.join(REF, "tools", "5_evaluation_bop_icp3d.py")).read()
    body = ast.parse(src).body
    fcn = [n for n in body if isinstance(n, ast.FunctionDef) and n.name == "fcn"][0]
    k_loop = [i for i, n in enumerate(body) if isinstance(n, ast.For) and isinstance(n.target, ast.Tuple)
              and [e.id for e in n.target.elts] == ["scene_id", "im_id", "obj_id_targets", "inst_counts"]][0]
    tail = body[k_loop + 1:]                       # the result-writing lines
    state = {"cur": None, "last": None, "union": None}
    log_est, log_icp, saved = [], [], {}
    rendered = {}
    by_key = {(im["scene_id"], im["im_id"]): im for im in ims}
    raw = raw_depth()

    inout = types.ModuleType("inout")
    inout.load_scene_camera = lambda path: {im["im_id"]: {"cam_K": K.copy(), "depth_scale": 1.0} for im in ims
                                            if path.endswith("/%06d/scene_camera.json" % im["scene_id"])}

    def load_im(path):
        sid, iid = int(path.split("/")[-3]), int(path.split("/")[-1].split(".")[0])
        state["cur"] = by_key[(sid, iid)]
        return np.zeros((H, W, 3), np.uint8)

    inout.load_im = load_im
    inout.load_depth = lambda path: raw.copy()

    def save_bop_results(path, results):
        saved["path"] = path
        saved["rows"] = results

    inout.save_bop_results = save_bop_results

    def get_rcnn_detection(image_t, model):
        im = state["cur"]
        n = len(im["rois"])
        return (np.array(im["rois"], np.int64).reshape(n, 4), np.zeros(n, np.int64), np.array(im["obj_ids"]),
                np.array(im["scores"], np.float64), np.stack(im["masks"], 2) if n else np.zeros((H, W, 0), bool))

    class Est:
        def __init__(self, model_id):
            self.model_id = model_id

        def est_pose(self, image_t, roi):
            # rois repeat in an image, so the outcome is looked up by the loop's own r_id, read from the caller's frame
            im = state["cur"]
            r_id = sys._getframe(1).f_locals["r_id"]
            assert list(roi) == list(im["rois"][r_id])
            oc = im["out"].setdefault((r_id, self.model_id), dict(EST_FAIL))      # not scripted: est_pose fails
            log_est.append([im["scene_id"], im["im_id"], r_id, self.model_id])
            state["last"] = (r_id, self.model_id)
            if oc["est"] == "fail":
                return None, None, 0, 0, -1, None
            return None, np.zeros((H, W), bool), np.array(oc["R_est"]), np.array(oc["t_est"]), 0.5, None

    def icp_refinement(pts_tgt, obj_model, rot_pred, tra_pred, cam_K, ren, union_mask):
        im = state["cur"]
        oc = im["out"][state["last"]]
        log_icp.append([im["scene_id"], im["im_id"], state["last"][0], state["last"][1], int(np.sum(union_mask))])
        state["union"] = np.asarray(union_mask, bool).copy()
        if oc["icp"] == "fail":
            return np.eye(4), -1
        return np.array(oc["tf"], np.float64), 0.0

    def render_obj(obj_model, rot, tra, cam_K, ren):
        im = state["cur"]
        oc = im["out"][state["last"]]
        depth_t = raw / 1000 * 1.0
        inl = first_k(state["union"], oc["k"], oc["last"])
        d = np.where(inl, depth_t.astype(np.float64), depth_t.astype(np.float64) + 0.5)
        rendered[(im["scene_id"], im["im_id"]) + state["last"]] = d
        return None, d

    targets = [(im["scene_id"], im["im_id"], list(im["targets"]), list(im["counts"])) for im in ims]
    ns = {"np": np, "os": os, "time": __import__("time"), "inout": inout, "get_rcnn_detection": get_rcnn_detection,
          "obj_pix2pose": [Est(m) for m in MODEL_IDS], "model_ids_list": list(MODEL_IDS), "obj_models": [None] * len(MODEL_IDS),
          "icp_refinement": icp_refinement, "render_obj": render_obj, "getXYZ": lambda d, **k: np.zeros(d.shape + (3,), np.float32),
          "get_normal": lambda d, **k: np.zeros(d.shape + (3,), np.float32), "target_list": targets, "prev_sid": -1,
          "dummy_run": False, "gpu_rendering": False, "ren": None, "model": None, "test_dir": "/T", "img_type": "rgb", "dataset": "ycbv",
          "detect_type": "rcnn", "score_type": 2, "task_type": 2, "im_height": H, "im_width": W, "result_dataset": [],
          "output_dir": "/out", "vis": False}
    code = compile(ast.Module([fcn, body[k_loop]] + tail, []), "icp3d_loop", "exec")
    with redirect_stdout(io.StringIO()):
        exec(code, ns)
    return saved, log_est, log_icp, rendered


def main(ref):
    ims = scenario()
    saved, log_est, log_icp, rendered = run_reference(ref, ims)
    out_ims = []
    for im in ims:
        outs = []
        for (r, o), oc in sorted(im["out"].items()):
            e = dict(oc, r_id=r, obj_id=o)
            key = (im["scene_id"], im["im_id"], r, o)
            if key in rendered:
                e["render"] = f32_b64(rendered[key].astype(np.float32))       # 1.0 and 1.5: exact in float32
            outs.append(e)
        out_ims.append({k: im[k] for k in ("scene_id", "im_id", "targets", "counts", "rois", "obj_ids", "scores")} |
                       {"masks": [u8_b64(m) for m in im["masks"]], "outcomes": outs})
    rows = [{"scene_id": int(r["scene_id"]), "im_id": int(r["im_id"]), "obj_id": int(r["obj_id"]), "score": float(r["score"]),
             "R": np.asarray(r["R"], np.float64).reshape(-1).tolist(), "t": np.asarray(r["t"], np.float64).reshape(-1).tolist()}
            for r in saved["rows"]]
    fx = {"H": H, "W": W, "K": K.tolist(), "depth_scale": 1.0, "task_type": 2, "raw_depth": f32_b64(raw_depth()),
          "output_path": saved["path"], "images": out_ims, "rows": rows, "est_pose_calls": log_est, "icp_calls": log_icp}
    json.dump(fx, open(os.path.join(HERE, "reference_icp3d.json"), "w"))
    print("%d rows, %d est_pose calls, %d ICP calls" % (len(rows), len(log_est), len(log_icp)))


if __name__ == "__main__":
    main(sys.argv[1])
