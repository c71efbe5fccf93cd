"""Time of one 50-sample training batch (runtime.train_patch_batch): 128-px patches on 480 x 640 backgrounds,
imsize 128, colour stage on.  Warm-up, then REPS calls bracketed by events on the context's stream and by the host clock; beside it
the float64 restatement tests/train_ref.py on the same batch over 16 processes.  Writes profiles/train_batch_time.txt.

    python tools/time_train_batch.py [--no-cpu]

The per-kernel split comes from a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/time_train_batch.py --no-cpu
"""
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N, REPS, WARM = 50, 20, 3


def make_batch():
    from pix2pose_amd import runtime
    rs = np.random.RandomState(0)
    y, x = np.mgrid[0:128, 0:128]
    inside = ((y - 63.5) / 56) ** 2 + ((x - 63.5) / 52) ** 2 < 1
    patches, backs, draws = [], [], []
    random.seed(0)
    for k in range(N):
        p = rs.randint(0, 256, (128, 128, 6)).astype(np.uint8)
        p[..., 3:6] = np.where(inside[..., None], np.maximum(p[..., 3:6], 1), 0)
        patches.append(p)
        backs.append(rs.randint(0, 256, (480, 640, 3)).astype(np.uint8))
        draws.append(runtime.train_draws(random, p.shape, backs[-1].shape, k))
    colours = runtime.train_colours(np.random.default_rng(0), N)
    for c in colours:
        c["noise_scale"] = 0.0          # the restatement has no noise generator: the same records on both sides
    return patches, backs, draws, colours


def cpu_one(args):
    import train_ref as T
    return T.get_patch_pair(*args)[0].shape


def main():
    import torch
    from pix2pose_amd import runtime
    ctx = runtime.Context(0)
    patches, backs, draws, colours = make_batch()
    stream = torch.cuda.ExternalStream(ctx.stream)
    for _ in range(WARM):
        runtime.train_patch_batch(ctx, patches, backs, draws, colours, 128, device=True)
    ev, wall = [], []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(stream)
        runtime.train_patch_batch(ctx, patches, backs, draws, colours, 128, device=True)
        b.record(stream)
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    lines = ["train_patch_batch: %d samples, 128-px patches, 480x640 backgrounds, imsize 128, colour on, device outputs" % N,
             "events on the context stream (host marshalling and staging inside): median %.3f ms, min %.3f, max %.3f over %d calls"
             % (np.median(ev), min(ev), max(ev), REPS),
             "host clock per call: median %.3f ms, min %.3f, max %.3f" % (np.median(wall), min(wall), max(wall))]
    if "--no-cpu" not in sys.argv:
        import multiprocessing as mp
        jobs = [(patches[k], backs[k], draws[k], 128, colours[k]) for k in range(N)]
        with mp.get_context("spawn").Pool(16) as pool:
            pool.map(cpu_one, jobs[:16])
            t0 = time.perf_counter()
            pool.map(cpu_one, jobs)
            cpu = (time.perf_counter() - t0) * 1e3
        lines.append("float64 restatement (tests/train_ref.py) of the same batch over 16 processes: %.1f ms" % cpu)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out = os.environ.get("TRAIN_TIME_OUT", os.path.join(ROOT, "profiles", "train_batch_time.txt"))
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
