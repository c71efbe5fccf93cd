"""Wall time per image of the RGB-D evaluation on one synthetic 32-image chunk at 640 x 480, about 8 detections per image (objects 1
and 2, one duplicated detection per image), through the two routes the end-to-end test compares:
  device -- eval_bop_icp.run (frames, union / inlier masks and occupancy on the device, batched est_pose and refine, resolve kernel);
  host   -- tests/rgbd_ref.host_chain (host-darkened frames, est_pose_batch and refine_depth_batch per candidate, the numpy walk).
Each route runs once to warm up and is then timed (median of --repeat).  Prints one JSON line; --out writes it too.

    python tools/time_eval_icp.py [--repeat 3] [--out profiles/eval_icp_time.json]"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import depth_ref as D
    import rgbd_ref as RR
    import test_rgbd_gpu as T
    from pix2pose_amd import eval_bop_icp as E, runtime, synthetic, weights as Wt
    ctx = runtime.Context(0, max_batch=64, winograd="always")
    mesh = runtime.Mesh(ctx, *D.l_mesh(8))
    tmp = Path(tempfile.mkdtemp())
    dump, inject, host = T.synthetic_dump(ctx, mesh, tmp, n_img=a.images, dets_per_image=7, seed=3)
    n_det = sum(len(im["rois"]) for im in dump["images"])
    cfg = dict(T.CFG, batch_images=a.images)

    def device():
        return E.run(cfg, "ycbv", dump, base_dir=str(tmp), batch_images=a.images, inject=inject, write_csv=False)

    gen = runtime.Generator(Wt.synthetic_weights("resnet50", 1), "resnet50", ctx)
    spec = runtime.ObjectSpec(gen, synthetic.OBJ_PARAM, T.CFG["outlier_th"], T.CFG["inlier_th"])
    inj = dict(inject, row={(int(i), int(r)): k for k, (i, r) in enumerate(inject["key"])})

    def hostr():
        return RR.host_chain(ctx, [spec, spec], [mesh, mesh], host, task_type=2, inject=inj, anti_aliasing="0.14")[0]

    out = {"images": a.images, "detections": n_det, "H": 480, "W": 640}
    rows = {}
    for name, fn in (("device", device), ("host", hostr)):
        rows[name] = fn()
        ts = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[name + "_ms_per_image"] = 1000 * float(np.median(ts)) / a.images
    out["rows"] = len(rows["device"])
    out["rows_equal"] = [(r["obj_id"], r["score"]) for r in rows["device"]] == [(r["obj_id"], r["score"]) for r in rows["host"]]
    out["note"] = ("device: includes the driver's setup per run (context, generators, meshes, frame and depth reads from .npy); "
                   "host: the per-candidate loop only, with the networks already loaded")
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
