"""Wall time of the depth refinement at 640 x 480: p2p_refine_depth_batch (ICP inputs, point-to-plane ICP, refined pose, render and
score) for 1, 32 and 256 jobs over 4 frames, with the iterations per job; and p2p_icp_batch alone on the same point sets.  The only CPU
comparison is the numpy restatement tests/icp_ref.py (not OpenCV), timed on one job.  Run under
`rocprofv3 --kernel-trace --stats -- python tools/time_refine.py` for the split between the nearest-neighbour (icp_nn_*), selection
(icp_select_kernel, icp_picky_kernel), solve (icp_solve_kernel), grid, ICP-input and score kernels."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import depth_ref as D  # noqa: E402
import icp_ref as I  # noqa: E402
from pix2pose_amd.runtime import Context, Mesh, icp_batch, icp_inputs_batch, refine_depth_batch, render_depth_batch  # noqa: E402

H, W, REPS = 480, 640, 5
ctx = Context(0, max_batch=8)
v, t = D.l_mesh(32)
mesh = Mesh(ctx, v, t)
rs = np.random.RandomState(0)
jj, ii = np.meshgrid(np.arange(W), np.arange(H))
depths, poses = [], []
for k in range(4):
    R = D.rot(0, 20 + 7 * k) @ D.rot(1, -25 + 11 * k)
    tt = np.array([-40.0 + 25 * k, 20.0 - 10 * k, 650.0 + 30 * k])
    obj = render_depth_batch(ctx, [mesh], [{"mesh": 0, "camK": D.K_640, "R": R, "t": tt}], H, W)[0]
    wall = (1.1 + 0.05 * np.sin(jj / 31.0) * np.cos(ii / 23.0)).astype(np.float32)
    d = np.where(obj > 0, obj + rs.normal(scale=0.0005, size=obj.shape).astype(np.float32), wall).astype(np.float32)
    d[rs.rand(H, W) < 0.03] = 0
    m = obj > 0
    for _ in range(1):                                   # the detector mask: the silhouette grown by 1 px
        m[1:] |= m[:-1]; m[:-1] |= m[1:]; m[:, 1:] |= m[:, :-1]; m[:, :-1] |= m[:, 1:]
    depths.append(d)
    poses.append((R, tt, (m & (d > 0.2)).astype(np.uint8)))
jobs = []
for k in range(256):
    R, tt, um = poses[k % 4]
    jobs.append({"mesh": 0, "image": k % 4, "camK": D.K_640, "R": D.rot(1, rs.uniform(-4, 4)) @ R, "t": tt + rs.uniform(-10, 10, 3),
                 "union_mask": um})
print("mesh: %d triangles; %d x %d" % (len(t), W, H))


def timed(name, n, fn):
    fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    print("%-12s %3d jobs %9.1f us each (median of %d calls, %.2f ms per call)" % (name, n, 1e6 * np.median(ts) / n, REPS,
                                                                                 1e3 * np.median(ts)))
    return out


for n in (1, 32, 256):
    out = timed("refine", n, lambda: refine_depth_batch(ctx, [mesh], depths, jobs[:n]))
    its = np.array([o["iterations"][:2] for o in out])
    print("    status 0: %d of %d; iterations per job (level 1, level 0): mean %.1f / %.1f, max %d / %d; source points %d, target %d" % (
        sum(o["status"] == 0 for o in out), n, its[:, 1].mean(), its[:, 0].mean(), its[:, 1].max(), its[:, 0].max(),
        sum(o["n_src"] for o in out), sum(o["n_tgt"] for o in out)))
    ins = icp_inputs_batch(ctx, [mesh], depths, jobs[:n])
    timed("inputs", n, lambda: icp_inputs_batch(ctx, [mesh], depths, jobs[:n]))
    timed("icp", n, lambda: icp_batch(ctx, ins))
t0 = time.perf_counter()
I.icp(ins[0]["src"], ins[0]["tgt"])
print("numpy restatement (tests/icp_ref.py), one job of %d / %d points: %.1f ms" % (len(ins[0]["src"]), len(ins[0]["tgt"]),
                                                                                   1e3 * (time.perf_counter() - t0)))
