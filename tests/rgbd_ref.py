"""numpy restatement of the per-image loop of tools/5_evaluation_bop_icp3d.py :331-540.

prepare(): the frame preparation of :360-370.  walk(): the two-round walk of :394-510 over rois and candidates, driven by an outcome
function that stands for est_pose, the t_z gate, the union gate and the refinement of one (round, roi, object) candidate.  It
returns the result rows in append order and the candidates in the order the reference evaluates them.  superset(): the candidates
the batched driver evaluates (pix2pose_amd.eval_bop_icp), so that a test can hold the walk over it to the on-demand walk."""
import numpy as np


def prepare(raw, depth_scale, rgb):
    """-> depth_t (float32), depth_valid (bool), frame (float32 H x W x 3), exactly numpy's expressions of :360-370."""
    depth_t = np.asarray(raw).astype(np.float32) / 1000 * np.float32(depth_scale)
    depth_t = depth_t.astype(np.float32)
    depth_t_zero_nan = np.nan_to_num(depth_t)
    with np.errstate(invalid="ignore"):
        depth_valid = np.logical_and(depth_t > np.float32(0.2), depth_t < np.float32(2.2))
    rgb_valid = np.logical_or(depth_valid, depth_t_zero_nan == 0)
    image_t = np.asarray(rgb).astype(np.float32)
    image_t[np.invert(rgb_valid)] = np.float32(0.1) * image_t[np.invert(rgb_valid)]
    return depth_t, depth_valid, image_t


def mask_iou(occ, mask):
    """:405, :430: numpy's ratio of two integer sums (0 / 0 is NaN)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float64(np.sum(np.logical_and(occ, mask))) / np.float64(np.sum(np.logical_or(occ, mask)))


def walk(obj_id_targets, inst_counts, rois, obj_ids, scores, masks, outcome, shape):
    """rois [n][4], obj_ids, scores (detector), masks [n][H][W] bool.  outcome(rounds, r_id, obj_id) -> dict with "stage":
    "est" (est_pose failed), "near" (t_z < 0.2 m), "union" (union <= 30), "refine" (ICP -1) or "ok", and for "ok": R, t, fcn, ratio,
    inlier_mask.  -> (rows: list of dict obj_id, score, R, t, round, r_id in append order, evaluated: [(rounds, r_id, obj_id)])."""
    inst_count_pred = np.zeros(len(inst_counts))
    occupancy = np.zeros(shape, bool)
    roi_used, rows, evaluated = [], [], []
    inlier_mask = None
    for rounds in range(2):
        for r_id, roi in enumerate(rois):
            if rounds == 1 and r_id in roi_used:
                continue
            if roi[0] == -1 and roi[1] == -1:
                continue
            obj_id = obj_ids[r_id]
            if rounds == 0 and obj_id not in obj_id_targets:
                continue
            elif rounds == 0:
                mask_from_detect = masks[r_id]
                if mask_iou(occupancy == obj_id, mask_from_detect) > 0.7:
                    continue
                obj_id_, obj_gt_no_ = [obj_id], [obj_id_targets.index(obj_id)]
            else:
                obj_id_, obj_gt_no_ = [], []
                for g, o in enumerate(obj_id_targets):
                    if inst_count_pred[g] < inst_counts[g]:
                        obj_id_.append(o)
                        obj_gt_no_.append(g)
                if len(obj_id_) == 0:
                    break
                mask_from_detect = masks[r_id]
                if mask_iou(occupancy != 0, mask_from_detect) > 0.7:
                    continue
            best_obj_id, best_gt_no, best_score, best_R, best_t, best_ratio = 0, 0, 0, 0, 0, 0
            for o, g in zip(obj_id_, obj_gt_no_):
                evaluated.append((rounds, r_id, o))
                oc = outcome(rounds, r_id, o)
                if oc["stage"] != "ok":
                    continue
                inlier_mask = oc["inlier_mask"]
                score = (scores[r_id] if rounds == 0 else 0.001) * oc["fcn"]
                ratio = oc["ratio"]
                if best_score < score:
                    best_obj_id, best_gt_no, best_score, best_R, best_t, best_ratio = o, g, score, oc["R"], oc["t"], ratio
            if best_score > 0:
                if rounds == 0 or best_ratio > 0.5:
                    inst_count_pred[best_gt_no] += 1
                    occupancy[inlier_mask] = best_obj_id
                    roi_used.append(r_id)
                rows.append({"obj_id": best_obj_id, "score": best_score, "R": best_R, "t": best_t, "round": rounds, "r_id": r_id})
    return rows, evaluated


def superset_round0(obj_id_targets, rois, obj_ids):
    return [(r, obj_ids[r]) for r, roi in enumerate(rois) if not (roi[0] == -1 and roi[1] == -1) and obj_ids[r] in obj_id_targets]


def superset_round1(obj_id_targets, inst_counts, rois, roi_used, inst_count_pred):
    missing = [o for g, o in enumerate(obj_id_targets) if inst_count_pred[g] < inst_counts[g]]
    return [(r, o) for r, roi in enumerate(rois) if r not in roi_used and not (roi[0] == -1 and roi[1] == -1) for o in missing]


def state_after_round0(obj_id_targets, inst_counts, rows):
    """roi_used and inst_count_pred after round 0, from its rows (a round-0 row always counts, :500-506)."""
    pred = np.zeros(len(inst_counts))
    used = []
    for r in rows:
        if r["round"] == 0:
            pred[obj_id_targets.index(r["obj_id"])] += 1
            used.append(r["r_id"])
    return used, pred


def host_chain(ctx, specs, meshes, images, task_type=2, inject=None, anti_aliasing="0.14", icp_params=None):
    """The sequential loop with the library's per-call entry points, one candidate at a time on demand: est_pose_batch on the
    host-darkened float32 frame, the t_z and union gates on the host, refine_depth_batch with a host union mask, then walk() and
    eval_bop.rank_image_results.  images: dicts scene_id, im_id, gi, rgb, raw, depth_scale, K, targets, counts, rois, obj_ids, scores,
    masks [n][H][W]; specs / meshes indexed by model index = position of the object id in model_ids.  -> (rows, evaluated)."""
    import torch
    from pix2pose_amd import runtime
    from pix2pose_amd.eval_bop import rank_image_results
    model_ids = images[0]["model_ids"] if images else []
    rows, evaluated = [], []
    for im in images:
        depth_t, depth_valid, frame = prepare(im["raw"], im["depth_scale"], im["rgb"])
        cache = {}

        def outcome(rounds, r, o, im=im, depth_t=depth_t, depth_valid=depth_valid, frame=frame, cache=cache):
            if (r, o) in cache:
                return cache[(r, o)]
            extra, held = {}, None
            if inject is not None:
                k = inject["row"][(im["gi"], r)]
                held = (torch.from_numpy(np.ascontiguousarray(inject["inject1"][k:k + 1])).cuda(ctx.device),
                        torch.from_numpy(np.ascontiguousarray(inject["inject2"][k:k + 1])).cuda(ctx.device))
                torch.cuda.synchronize(ctx.device)
                extra = dict(inject1=held[0].data_ptr(), inject2=held[1].data_ptr(), inject_slots=int(held[1].shape[1]))
            m = model_ids.index(o)
            p = runtime.est_pose_batch(ctx, specs, [frame], [(0, m, [int(v) for v in im["rois"][r]], im["K"])],
                                       anti_aliasing=anti_aliasing, **extra)[0][0]
            del held
            if int(p.status) != 0:
                oc = {"stage": "est"}
            elif p.t[2] / 1000 < 0.2:
                oc = {"stage": "near"}
            else:
                union = np.asarray(im["masks"][r], bool) & depth_valid
                if union.sum() <= 30:
                    oc = {"stage": "union"}
                else:
                    res, inl = runtime.refine_depth_batch(ctx, meshes, [depth_t], [{"image": 0, "mesh": m, "camK": im["K"],
                                                          "R": np.array(p.R[:]).reshape(3, 3), "t": np.array(p.t[:]),
                                                          "union_mask": union}], inlier_masks=True, **(icp_params or {}))
                    q = res[0]
                    oc = ({"stage": "refine"} if q["status"] != 0 else
                          {"stage": "ok", "R": q["R"], "t": q["t"], "fcn": q["fcn"], "ratio": q["ratio"], "inlier_mask": inl[0],
                           "R_est": np.array(p.R[:]).reshape(3, 3), "t_est": np.array(p.t[:])})
            cache[(r, o)] = oc
            return oc

        res, ev = walk(im["targets"], im["counts"], im["rois"], im["obj_ids"], im["scores"], [np.asarray(m, bool) for m in im["masks"]],
                       outcome, depth_t.shape)
        evaluated.append((im, ev, cache))
        rows += rank_image_results(res, im["targets"], im["counts"], '2' if int(task_type) == 2 else int(task_type), im["scene_id"],
                                   im["im_id"], 0.0)
    return rows, evaluated
