"""Wall time of depth back-projection, normals and the ICP point sets at 640 x 480: p2p_depth_points_batch (whole frames, host
buffers in and out) for 1 and 8 images, and p2p_icp_inputs_batch (scene points of the named frames, target points, render, source
points with normals, centroids) for 1, 32 and 256 jobs over 4 frames.  Run under
`rocprofv3 --kernel-trace --stats -- python tools/time_normals.py` for the split between the fill, Gaussian, normal, compaction and
raster kernels."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import depth_ref as D  # noqa: E402
from pix2pose_amd.runtime import Context, Mesh, depth_points_batch, icp_inputs_batch  # noqa: E402

H, W, REPS = 480, 640, 5
ctx = Context(0, max_batch=8)
v, t = D.l_mesh(32)
mesh = Mesh(ctx, v, t)
rs = np.random.RandomState(0)
jj, ii = np.meshgrid(np.arange(W), np.arange(H))
depths = []
for k in range(8):
    d = (0.9 + 0.2 * np.sin(jj / (20.0 + k)) * np.cos(ii / 17.0)).astype(np.float32)
    d[rs.rand(H, W) < 0.05] = 0                          # sensor dropout: the fill has work to do
    d[100 + 10 * k:160 + 10 * k, 200:300] = 0
    depths.append(d)
jobs = []
for k in range(256):
    R = D.rot(0, rs.uniform(-180, 180)) @ D.rot(1, rs.uniform(-180, 180))
    z = rs.uniform(0.4, 1.2)
    tt = np.array([rs.uniform(-0.15, 0.15) * z, rs.uniform(-0.1, 0.1) * z, z]) * 1000.0      # mm
    mask = np.zeros((H, W), np.uint8)
    mask[150:330, 220:420] = 1
    jobs.append({"mesh": 0, "image": k % 4, "camK": D.K_640, "R": R, "t": tt, "union_mask": mask & (depths[k % 4] > 0.2)})
print("mesh: %d triangles; %d x %d" % (len(t), W, H))


def timed(name, n, fn):
    fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    print("%-12s %3d %-7s %9.1f us each (median of %d calls, %.2f ms per call)" % (name, n, "images" if name == "points" else "jobs",
                                                                                    1e6 * np.median(ts) / n, REPS, 1e3 * np.median(ts)))
    return out


for n in (1, 8):
    timed("points", n, lambda: depth_points_batch(ctx, depths[:n], [D.K_640] * n))
for n in (1, 32, 256):
    out = timed("icp_inputs", n, lambda: icp_inputs_batch(ctx, [mesh], depths[:4], jobs[:n]))
    print("    status 0: %d of %d, source points %d, target points %d" % (sum(o["status"] == 0 for o in out), n,
                                                                        sum(len(o["src"]) for o in out), sum(len(o["tgt"]) for o in out)))
