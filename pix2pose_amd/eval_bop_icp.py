"""Counterpart of the reference's RGB-D BOP evaluation driver (tools/5_evaluation_bop_icp3d.py): est_pose on the depth-darkened
frame, point-to-plane ICP refinement against the sensor depth, the depth score, and the occupancy walk that assigns each Mask R-CNN
roi to at most one object.

CLI as eval_bop: ``python -m pix2pose_amd.eval_bop_icp <gpu_id> <cfg.json> <dataset> [detections.json]``; the same pre-dumped
detection stream (a dump dict, or a COCO-style list for cfg["dataset_dir"], read through bop_dataset.build_dump(with_depth=True)),
plus per image "depth" (16-bit .png, itodd .tif, or .npy) and "depth_scale", top-level "meshes" {obj id: .ply}, and a detector mask
("masks" or "segmentations") for every detection.  Only the score_type 2 / Mask R-CNN branch of the reference defines its score
(:455-489); anything else is refused, and so is WORLD_SIZE > 1.

Execution.  The reference walks one roi at a time; here a chunk of cfg["batch_images"] images (default 32) goes through the device
in two rounds.  Round 0 evaluates every roi of a target object (the candidates the reference can evaluate in round 0 follow from
the dump alone); round 1 evaluates every roi left unused by round 0 against every target still missing after round 0 (the missing
set only shrinks during round 1, so this is a superset of what the reference evaluates).  The resolve kernel then walks each image in
the reference's order and reads only the outcomes of the candidates the reference evaluates.  This is exact on one condition: a
candidate's est_pose and refine results must not depend on what else is in the batch.  Refine is bit-identical alone and in a batch;
for est_pose the context runs the 5x5 layers with one Winograd form at every pass size (set_winograd("always")), since under the
default "auto" a sample's bits depend on the size of its generator pass.

Rules kept from the reference: float32 frame preparation (:360-370), no candidate limiting (cand_factor read and not
used, :413-415), the bool occupancy (obj 1 is skipped by its own earlier detections in round 0, other ids never are), the occupancy
update with the inlier mask of the roi's LAST scored candidate (:476, :506), best_ratio > 0.5 in round 1, and ViVo truncation for
task_type 2 (task_type is an int here, :169).  Not reproduced: the dummy_run warm-up calls, the dead norm_score branch, gpu_rendering.
"""
from __future__ import annotations

import json
import os
import time

import numpy as np

from .eval_bop import (FramePrefetcher, resize_generation_of, group_targets, model_params_to_obj_param, outlier_thresholds,
                       output_name, rank_image_results, save_bop_results)


def check_config(cfg: dict, detect_type: str = "rcnn"):
    """The branches of :455-489 this driver reproduces; raises ValueError with the reason otherwise."""
    if int(cfg["score_type"]) != 2:
        raise ValueError("eval_bop_icp: score_type %r is not supported: the reference's depth loop defines its score only for "
                         "score_type 2 with Mask R-CNN detections (tools/5_evaluation_bop_icp3d.py:455-489)" % cfg["score_type"])
    if detect_type != "rcnn":
        raise ValueError("eval_bop_icp: detection_pipeline %r is not supported: the depth score needs Mask R-CNN masks "
                         "(tools/5_evaluation_bop_icp3d.py:455-489)" % detect_type)


def check_world():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("eval_bop_icp: WORLD_SIZE > 1 -- multi-GPU sharding of the RGB-D driver is not supported")


def load_depth(path):
    """A depth frame in the sensor's unit: uint16 (16-bit .png / .tif) or float32 (.npy / float .tif)."""
    if path.endswith(".npy"):
        a = np.load(path)
    else:
        try:
            from PIL import Image
        except ImportError as e:  # pragma: no cover
            raise RuntimeError("reading %s needs Pillow; dump depth frames as .npy instead" % path) from e
        a = np.array(Image.open(path))
    if np.issubdtype(a.dtype, np.integer):
        if a.min(initial=0) < 0 or a.max(initial=0) > 65535:
            raise ValueError("depth frame %s does not fit 16 bits" % path)
        return a.astype(np.uint16)
    return a.astype(np.float32)


def image_masks(im, base_dir, n, shape):
    """Detector masks [n, H, W] bool of a dump image; every detection must have one."""
    if n == 0:
        return np.zeros((0,) + shape, bool)
    if im.get("masks"):
        m = np.load(os.path.join(base_dir, im["masks"]))
        if m.shape[:2] != shape or m.shape[2] != n:
            raise ValueError("masks of scene %s image %s have shape %r, expected %r" % (im["scene_id"], im["im_id"], m.shape, shape + (n,)))
        return np.moveaxis(m != 0, 2, 0)
    segs = im.get("segmentations")
    if segs is None or len(segs) != n or any(s is None for s in segs):
        raise ValueError("eval_bop_icp needs a detector mask for every detection (scene %s image %s)" % (im["scene_id"], im["im_id"]))
    from .bop_dataset import rle_decode
    out = np.stack([rle_decode(s) != 0 for s in segs])
    if out.shape[1:] != shape:
        raise ValueError("masks of scene %s image %s have shape %r, frame %r" % (im["scene_id"], im["im_id"], out.shape[1:], shape))
    return out


def round0_candidates(targets, rois, obj_ids):
    """(r_id, obj_id) the reference can evaluate in round 0 (:397-416): every valid roi of a target object."""
    return [(r, int(obj_ids[r])) for r, roi in enumerate(rois) if not (roi[0] == -1 and roi[1] == -1) and obj_ids[r] in targets]


def round1_candidates(targets, inst_counts, rois, roi_used, inst_pred):
    """A superset of what the reference evaluates in round 1 (:417-433): every valid roi not used in round 0 against every target
    still missing after round 0."""
    missing = [int(o) for g, o in enumerate(targets) if inst_pred[g] < inst_counts[g]]
    return [(r, o) for r, roi in enumerate(rois) if not roi_used[r] and not (roi[0] == -1 and roi[1] == -1) for o in missing]


def run(cfg: dict, dataset: str, dump: dict, device: int = 0, base_dir: str = ".", batch_images: int = 32, detect_type: str = "rcnn",
        inject=None, write_csv: bool = True, icp_params=None):
    """Evaluate a pre-dumped detection stream with depth.  Returns the result rows (also written as CSV when cfg['path_to_output']
    is set).  inject (tests): {"key": [N, 2] (image position in the target list, detection index), "inject1", "inject2"} -- decoder
    maps that replace the generator output of the listed detections, as in eval_bop.run."""
    from . import _lib, runtime, weights as W
    check_world()
    check_config(cfg, detect_type)
    backbone = cfg.get("backbone", "paper")
    model_ids = [int(m) for m in dump["model_ids"]]
    th_o = outlier_thresholds(cfg, len(model_ids))
    th_i = cfg["inlier_th"]
    task_type = int(cfg["task_type"])                                        # :169
    rank_task = '2' if task_type == 2 else task_type
    float(cfg.get("cand_factor", 1.0))                                       # read and not used (:413-415 are commented out)
    ctx = runtime.Context(device, max_batch=int(cfg.get("generator_chunk", 256)), winograd="always")
    specs, meshes = [], []
    for m, mid in enumerate(model_ids):
        wfn = dump["weights"][str(mid)]
        if not wfn.startswith(("synthetic:", "trained-like:")):
            wfn = os.path.join(base_dir, wfn)
        gen = runtime.Generator(W.load_weights(wfn, backbone), backbone, ctx)
        specs.append(runtime.ObjectSpec(gen, model_params_to_obj_param(dump["norm_factor"][str(mid)]), th_o[m], th_i))
        meshes.append(runtime.Mesh.from_ply(ctx, os.path.join(base_dir, dump["meshes"][str(mid)])))
    aa = resize_generation_of(cfg)
    rg = runtime.Rgbd(ctx)
    by_image = {(im["scene_id"], im["im_id"]): im for im in dump["images"]}
    tlist = [t + [gi] for gi, t in enumerate(group_targets(dump["targets"]))]
    inject_row = {(int(a), int(b)): i for i, (a, b) in enumerate(inject["key"])} if inject is not None else None
    loader = FramePrefetcher(int(cfg.get("loader_threads", 8)))
    rows = []

    def est_pose(chunk_imgs, cands):
        """cands: (chunk image, r_id, obj_id) -> list of (code or None, R, t) per candidate."""
        dets = [(ci, model_ids.index(o), [int(v) for v in chunk_imgs[ci]["rois"][r]], chunk_imgs[ci]["K"]) for ci, r, o in cands]
        extra, held = {}, None
        if inject is not None:
            import torch
            idx = [inject_row[(chunk_imgs[ci]["gi"], r)] for ci, r, _o in cands]
            held = (torch.from_numpy(np.ascontiguousarray(inject["inject1"][idx])).cuda(device),
                    torch.from_numpy(np.ascontiguousarray(inject["inject2"][idx])).cuda(device))
            torch.cuda.synchronize(device)
            extra = dict(inject1=held[0].data_ptr(), inject2=held[1].data_ptr(), inject_slots=int(held[1].shape[1]))
        poses, _ = runtime.est_pose_batch(ctx, specs, [rg.image(i) for i in range(len(chunk_imgs))], dets, anti_aliasing=aa, **extra)
        del held
        return poses

    def evaluate(chunk_imgs, cands):
        """est_pose, the t_z gate and refine of cands -> cand_ref per candidate (record index or a _lib.RGBD_* code)."""
        refs = [_lib.RGBD_NOT_EVALUATED] * len(cands)
        if not cands:
            rg.refine(meshes, [], [])
            return refs
        poses = est_pose(chunk_imgs, cands)
        jobs, midx = [], []
        for k, ((ci, r, o), p) in enumerate(zip(cands, poses)):
            if int(p.status) != 0:                                           # frac_inlier == -1 (:444-445)
                refs[k] = _lib.RGBD_EST_FAILED
            elif p.t[2] / 1000 < 0.2:                                        # :449-450
                refs[k] = _lib.RGBD_NEAR
            else:
                refs[k] = len(jobs)
                jobs.append({"image": ci, "mesh": model_ids.index(o), "camK": chunk_imgs[ci]["K"],
                             "R": np.array(p.R[:]).reshape(3, 3), "t": np.array(p.t[:])})
                midx.append(chunk_imgs[ci]["mask0"] + r)
        rg.refine(meshes, jobs, midx, raw=True, **(icp_params or {}))
        return refs

    def resolve_input(chunk_imgs, cands, refs):
        per = [[[] for _ in ci["rois"]] for ci in chunk_imgs]
        for (ci, r, o), ref in zip(cands, refs):
            per[ci][r].append((o, ref))
        return [{"targets": ci["targets"], "inst_counts": ci["counts"],
                 "rois": [{"obj": int(ci["obj_ids"][r]), "score": float(ci["scores"][r]),
                           "valid": not (roi[0] == -1 and roi[1] == -1), "mask": ci["mask0"] + r, "cands": per[k][r]}
                          for r, roi in enumerate(ci["rois"])]} for k, ci in enumerate(chunk_imgs)]

    for b0 in range(0, len(tlist), batch_images):
        chunk = tlist[b0:b0 + batch_images]
        loader.request([os.path.join(base_dir, by_image[(c[0], c[1])]["rgb"]) for c in tlist[b0 + batch_images:b0 + 2 * batch_images]
                        if (c[0], c[1]) in by_image])
        t1 = time.time()
        chunk_imgs, rgbs, depths, scales, masks, mask_image = [], [], [], [], [], []
        for scene_id, im_id, targets, counts, gi in chunk:
            im = by_image.get((scene_id, im_id))
            if im is None:
                continue
            rgb = loader.get(os.path.join(base_dir, im["rgb"]))
            if "depth" not in im or "depth_scale" not in im:
                raise ValueError("scene %s image %s has no depth / depth_scale in the dump (bop_dataset.build_dump(with_depth=True))"
                                 % (scene_id, im_id))
            d = load_depth(os.path.join(base_dir, im["depth"]))
            if d.shape != rgb.shape[:2]:
                raise ValueError("depth of scene %s image %s is %r, its frame %r" % (scene_id, im_id, d.shape, rgb.shape[:2]))
            n = len(im["rois"])
            m = image_masks(im, base_dir, n, d.shape)
            chunk_imgs.append({"scene_id": scene_id, "im_id": im_id, "targets": [int(t) for t in targets], "counts": [int(c) for c in counts],
                               "gi": gi, "rois": im["rois"], "obj_ids": [int(o) for o in im["obj_ids"]], "scores": im["scores"],
                               "K": np.array(im["cam_K"], np.float64).reshape(3, 3), "mask0": len(mask_image)})
            rgbs.append(rgb)
            depths.append(d)
            scales.append(float(im["depth_scale"]))
            masks.extend(m)
            mask_image.extend([len(rgbs) - 1] * n)
        if not chunk_imgs:
            continue
        if len({d.dtype for d in depths}) > 1:
            depths = [d.astype(np.float32) for d in depths]          # exact: a 16-bit value is a float32
        if len({d.shape for d in depths}) > 1:
            raise ValueError("the frames of a chunk must have one size")
        rg.load(rgbs, depths, scales, np.array(masks) if masks else [], mask_image)
        n_rois = sum(len(ci["rois"]) for ci in chunk_imgs)
        roi_used = np.zeros(max(n_rois, 1), np.int32)[:n_rois]
        inst_pred = np.zeros(sum(len(ci["targets"]) for ci in chunk_imgs), np.int32)
        # round 0: from the dump alone
        c0 = [(k, r, o) for k, ci in enumerate(chunk_imgs) for r, o in round0_candidates(ci["targets"], ci["rois"], ci["obj_ids"])]
        refs0 = evaluate(chunk_imgs, c0)
        rows0 = rg.resolve(0, resolve_input(chunk_imgs, c0, refs0), roi_used, inst_pred)
        # round 1: the superset after round 0
        c1, ro, to = [], 0, 0
        for k, ci in enumerate(chunk_imgs):
            nr, nt = len(ci["rois"]), len(ci["targets"])
            c1 += [(k, r, o) for r, o in round1_candidates(ci["targets"], ci["counts"], ci["rois"], roi_used[ro:ro + nr], inst_pred[to:to + nt])]
            ro += nr
            to += nt
        refs1 = evaluate(chunk_imgs, c1)
        rows1 = rg.resolve(1, resolve_input(chunk_imgs, c1, refs1), roi_used, inst_pred)
        dt = time.time() - t1
        n_all = max(len(c0) + len(c1), 1)
        ro = 0
        for k, ci in enumerate(chunk_imgs):
            nr = len(ci["rois"])
            res = [{"obj_id": int(w[0]), "score": float(w[1]), "R": w[2:11].reshape(3, 3).copy(), "t": w[11:14].copy()}
                   for rr in (rows0, rows1) for w in rr[ro:ro + nr] if w[0] != 0]
            ro += nr
            n_here = sum(1 for c in c0 + c1 if c[0] == k)
            rows.extend(rank_image_results(res, ci["targets"], ci["counts"], rank_task, ci["scene_id"], ci["im_id"], dt * n_here / n_all))
    loader.close()
    rg.close()
    for m in meshes:
        m.close()
    out_dir = cfg.get("path_to_output")
    if out_dir and write_csv:
        os.makedirs(out_dir, exist_ok=True)
        save_bop_results(os.path.join(out_dir, output_name(dataset)), rows)
    return rows


def main(argv):
    if len(argv) < 4:
        print("usage: python -m pix2pose_amd.eval_bop_icp <gpu_id> <cfg.json> <dataset> [detections.json]\n"
              "  detections.json: a dump dict with depth, depth_scale and meshes (module docstring), or a COCO-style detection list for\n"
              "  the BOP directory cfg['dataset_dir'] (bop_dataset.build_dump(with_depth=True)).")
        return 2
    check_world()
    device, cfg_fn, dataset = int(argv[1]), argv[2], argv[3]
    cfg = json.load(open(cfg_fn))
    detect_type = cfg.get("detection_pipeline", "rcnn")
    check_config(cfg, detect_type)
    det_fn = argv[4] if len(argv) > 4 else os.path.join(cfg["dataset_dir"], dataset, "detections_mi355.json")
    dump = json.load(open(det_fn))
    base_dir = os.path.dirname(os.path.abspath(det_fn))
    if isinstance(dump, list):
        from . import bop_dataset
        dump = bop_dataset.build_dump(cfg, dataset, dump, with_depth=True)
    inject = None
    if os.environ.get("P2P_EVAL_INJECT"):             # test hook, see run()
        with np.load(os.environ["P2P_EVAL_INJECT"]) as z:
            inject = {k: z[k] for k in ("key", "inject1", "inject2")}
    rows = run(cfg, dataset, dump, device=device, base_dir=base_dir, inject=inject, detect_type=detect_type,
               batch_images=int(cfg.get("batch_images", 32)))
    print("Saving %d results to %s" % (len(rows), os.path.join(cfg.get("path_to_output", "."), output_name(dataset))))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main(sys.argv))
