"""The RGB-D walk as this library restates it (tests/rgbd_ref.py, and eval_bop.rank_image_results for the ranking) against
tests/golden/reference_icp3d.json, which holds what the reference's own per-image loop (tools/5_evaluation_bop_icp3d.py :331-540)
produced with scripted detections, est_pose, ICP and render outcomes (tests/golden/make_reference_icp3d_vectors.py).  This pins the
bool occupancy, the last-scored mask, the ratio 0.5 edge, the IoU 0.7 edge, the round-1 recompute and break and ViVo truncation to
the reference's lines, not to this library's reading of them.

Bars: the evaluated-candidate log (est_pose calls) and the ICP call log exact; rows exact in order, object, R and t, scores to 1e-12
relative."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_ref as D  # noqa: E402
import rgbd_ref as RR  # noqa: E402
from golden.make_reference_normals_vectors import b64_f32, b64_u8  # noqa: E402


def load():
    return json.load(open(os.path.join(HERE, "golden", "reference_icp3d.json")))


def restated(G):
    from pix2pose_amd.eval_bop import rank_image_results
    H, W = G["H"], G["W"]
    raw = b64_f32(G["raw_depth"], (H, W))
    depth_t, depth_valid, _ = RR.prepare(raw, G["depth_scale"], np.zeros((H, W, 3), np.uint8))
    rows, est_log, icp_log = [], [], []
    for im in G["images"]:
        masks = [b64_u8(m, (H, W)).astype(bool) for m in im["masks"]]
        table = {(o["r_id"], o["obj_id"]): o for o in im["outcomes"]}
        key = (im["scene_id"], im["im_id"])

        def outcome(rounds, r, o, masks=masks, table=table, key=key):
            oc = table[(r, o)]
            est_log.append([*key, r, o])
            if oc["est"] == "fail":
                return {"stage": "est"}
            if np.array(oc["t_est"])[2] / 1000 < 0.2:
                return {"stage": "near"}
            union = masks[r] & depth_valid
            if union.sum() <= 30:
                return {"stage": "union"}
            icp_log.append([*key, r, o, int(union.sum())])
            if oc["icp"] == "fail":
                return {"stage": "refine"}
            tf = np.array(oc["tf"], np.float64)
            sc, inl = D.depth_score(b64_f32(oc["render"], (H, W)), depth_t, union)
            return {"stage": "ok", "R": tf[:3, :3], "t": tf[:3, 3] * 1000, "fcn": sc["fcn"], "ratio": sc["ratio"], "inlier_mask": inl}

        res, _ = RR.walk(im["targets"], im["counts"], im["rois"], im["obj_ids"], im["scores"], masks, outcome, (H, W))
        task = '2' if int(G["task_type"]) == 2 else int(G["task_type"])
        rows += rank_image_results(res, im["targets"], im["counts"], task, im["scene_id"], im["im_id"], 0.0)
    return rows, est_log, icp_log


def test_restatement_reproduces_the_reference_loop():
    G = load()
    rows, est_log, icp_log = restated(G)
    assert est_log == G["est_pose_calls"]
    assert icp_log == G["icp_calls"]
    assert len(rows) == len(G["rows"]) and len(rows) >= 8
    for a, b in zip(rows, G["rows"]):
        assert (a["scene_id"], a["im_id"], a["obj_id"]) == (b["scene_id"], b["im_id"], b["obj_id"])
        assert abs(a["score"] - b["score"]) <= 1e-12 * abs(b["score"])
        np.testing.assert_array_equal(np.asarray(a["R"]).reshape(-1), b["R"])
        np.testing.assert_array_equal(np.asarray(a["t"]).reshape(-1), b["t"])


def test_fixture_reaches_the_scenario():
    """The situations of make_reference_icp3d_vectors.py's scenario are in the recorded logs."""
    G = load()
    ev = [tuple(c) for c in G["est_pose_calls"]]
    assert (1, 1, 1, 1) in ev and ev.index((1, 1, 1, 1)) > ev.index((1, 1, 10, 1))   # obj-1 duplicate: only in round 1
    assert (1, 1, 3, 2) in ev                                                         # obj-2 duplicate: evaluated in round 0
    assert [c[4] for c in G["icp_calls"] if c[:4] == [1, 1, 7, 2]] == [31] and not any(c[:4] == [1, 1, 6, 2] for c in G["icp_calls"])
    assert (1, 2, 1, 4) not in ev and (1, 2, 3, 4) not in ev                          # skip by the last-scored mask; the break
    assert (2, 1, 2, 5) in ev                                                         # IoU exactly 0.7 does not skip
    assert sum(1 for r in G["rows"] if (r["scene_id"], r["im_id"]) == (2, 2)) == 1     # ViVo truncation
    assert not any((r["scene_id"], r["im_id"]) == (3, 1) for r in G["rows"])           # no result
