"""Wall time of the depth path per detection at 640 x 480: p2p_render_depth_batch and p2p_depth_score_batch (render + score,
host buffers in and out) for 1, 32 and 256 jobs of a 24.6k-triangle mesh.  Run under
`rocprofv3 --kernel-trace --stats -- python tools/time_depth.py` for the split between the raster, finish and score kernels."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import depth_ref as D  # noqa: E402
from pix2pose_amd.runtime import Context, Mesh, depth_score_batch, render_depth_batch  # noqa: E402

H, W, REPS = 480, 640, 5
ctx = Context(0, max_batch=8)
v, t = D.l_mesh(32)
mesh = Mesh(ctx, v, t)
rs = np.random.RandomState(0)
depths = [rs.uniform(0.3, 1.3, (H, W)).astype(np.float32) for _ in range(4)]
jobs = []
for k in range(256):
    R = D.rot(0, rs.uniform(-180, 180)) @ D.rot(1, rs.uniform(-180, 180))
    z = rs.uniform(0.4, 1.2)
    tt = np.array([rs.uniform(-0.15, 0.15) * z, rs.uniform(-0.1, 0.1) * z, z]) * 1000.0      # mm
    mask = np.zeros((H, W), np.uint8)
    mask[150:330, 220:420] = 1
    jobs.append({"mesh": 0, "image": k % 4, "camK": D.K_640, "R": R, "t": tt, "union_mask": mask})
print("mesh: %d triangles; %d x %d" % (len(t), W, H))
for n in (1, 32, 256):
    for name, fn in (("render", lambda: render_depth_batch(ctx, [mesh], jobs[:n], H, W)),
                     ("render+score", lambda: depth_score_batch(ctx, [mesh], depths, jobs[:n]))):
        fn()
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        print("%-13s jobs %3d: %9.1f us/detection (median of %d calls, %.2f ms per call)" % (name, n, 1e6 * np.median(ts) / n, REPS,
                                                                                            1e3 * np.median(ts)))
