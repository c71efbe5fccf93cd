"""Times p2p_render_xyz_batch for 1, 32 and 256 jobs of a ~25k-triangle mesh at 640 x 480 (run it under
``rocprofv3 --kernel-trace --stats`` for the per-kernel split; profiles/xyz_render_time.txt)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import depth_ref as D  # noqa: E402

from pix2pose_amd.runtime import Context, Mesh, render_xyz_batch  # noqa: E402
from pix2pose_amd.xyz_model import xyz_colors  # noqa: E402

H, W, K = 480, 640, D.K_640
ctx = Context(0, max_batch=8)
v, t = D.box_mesh([-60, -45, -30], [60, 45, 30], 46)          # 25 392 triangles
m = Mesh(ctx, v, t)
m.set_colors(xyz_colors(v)[0])
rs = np.random.RandomState(0)
for n in (1, 32, 256):
    jobs = [{"mesh": 0, "camK": K, "R": R, "t": tt} for R, tt in (D.random_pose(rs, K, H, W, 0.4, 1.0) for _ in range(n))]
    render_xyz_batch(ctx, [m], jobs, H, W)                     # grows the workspaces
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        render_xyz_batch(ctx, [m], jobs, H, W)
    dt = (time.perf_counter() - t0) / reps
    print("jobs %4d: %.3f ms per call, %.1f us per job (host buffers in and out, %d triangles)" % (n, dt * 1e3, dt * 1e6 / n, len(t)), flush=True)
