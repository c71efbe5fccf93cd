"""Output census: one `name sha256` line per workload, over the generator output and the est_pose_batch pose records.

Run it twice -- the library of this tree, and another build named through P2P_LIB -- and diff the two outputs: a refactor
that must not move a bit shows an empty diff.  The workloads are the smallest input counts that reach each conv kernel
(streaming route, Winograd thresholds and K splits, fused blocks and halo kernels, batched kernels, mixed-object groups).
"""
import hashlib
import sys

import numpy as np
import torch

from pix2pose_amd import synthetic, weights as W
from pix2pose_amd.runtime import Context, Generator, ObjectSpec, est_pose_batch


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    rs = np.random.RandomState(0)
    x_all = (rs.randint(0, 256, (72, 128, 128, 3)).astype(np.float32) - 128) / 128
    for wino in ("auto", "always", "off"):
        ctx = Context(0, max_batch=128, winograd=wino)
        for backbone in ("resnet50", "paper"):
            w = W.synthetic_weights(backbone, 1)
            for prec in ("f16x3", "f32"):
                if prec == "f32" and wino != "auto":
                    continue                       # the Winograd switch only touches split-f16 passes
                gen = Generator(w, backbone, ctx, precision=prec)
                for n in (1, 3, 5, 9, 24, 40, 72):
                    dec, prob = gen.predict(x_all[:n])
                    print("gen %s %s wino=%s n=%d %s" % (backbone, prec, wino, n, sha(dec, prob)), flush=True)
    # mixed-object batch (the group lookups) and the pose records, resize_anti_aliasing 0 and 1
    ctx = Context(0, max_batch=64)
    th_o, th_i = [0.2, 0.3, 0.35], 0.2
    gens = [Generator(W.synthetic_weights("resnet50", s), "resnet50", ctx) for s in (1, 2, 3)]
    for aa in (0, 1):
        sc = synthetic.make_scene(16, seed=7, bbox_side=(120, 220))      # crops larger than 128 px: the resize down-scales, so aa matters
        specs = [ObjectSpec(g, synthetic.OBJ_PARAM, th_o, th_i) for g in gens]
        dets = [(d[0], o, d[2], d[3]) for o in range(3) for d in sc["dets"]]
        poses, _ = est_pose_batch(ctx, specs, list(sc["images"]), dets, anti_aliasing=bool(aa))
        rec = np.array([[p.status] + list(np.array(p.R).reshape(-1)) + list(np.array(p.t).reshape(-1)) for p in poses], dtype=np.float64)
        print("pose mixed 3x16 aa=%d %s" % (aa, sha(rec)), flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    sys.exit(main())
