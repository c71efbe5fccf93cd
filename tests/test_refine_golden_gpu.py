"""p2p_refine_depth_batch against tests/golden/reference_refine.json: the reference's own icp_refinement (taken from its syntax tree,
with the ICP, rasteriser and inpaint restatements stubbed in; tests/golden/make_reference_refine_vectors.py) recorded tf, or the -1 of
its gates.  The GPU returns R = tf[:3, :3] and t = tf[:3, 3] * 1000 (icp3d.py :466-467): R within 1e-6, t within 1e-4 mm, iteration
and pair counts exact, and the gated jobs as status -1 / -2.  The bars are those of tests/test_refine_golden_cpu.py: the point sets
agree with the reference's own to about 3e-8 relative, and a wrong composition order is off by 6e-3 in R and 7 mm or more in t."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from golden.make_reference_normals_vectors import b64_f32, b64_u8  # noqa: E402

pytestmark = pytest.mark.gpu


def test_refine_reproduces_the_reference_tf():
    from pix2pose_amd import runtime
    G = json.load(open(os.path.join(HERE, "golden", "reference_refine.json")))
    H, W, K = G["H"], G["W"], np.array(G["K"])
    ctx = runtime.Context(0, max_batch=8)
    try:
        mesh = runtime.Mesh(ctx, np.array(G["mesh_verts"]), np.array(G["mesh_tris"]))
        jobs = [{"mesh": 0, "image": 0, "camK": K, "R": np.array(j["R"]), "t": np.array(j["t"]),
                 "union_mask": b64_u8(j["union_mask"], (H, W))} for j in G["jobs"]]
        got = runtime.refine_depth_batch(ctx, [mesh], [b64_f32(G["image"], (H, W))], jobs, **G["params"])
        for g, j in zip(got, G["jobs"]):
            assert (g["status"] != 0) == (j["status"] == -1), j["why"]
            if j["status"] == -1:
                assert g["status"] in (-1, -2) and np.array_equal(g["R"], np.array(j["R"])), j["why"]
                continue
            tf = np.array(j["tf"])
            assert g["iterations"] == j["iterations"] and g["pairs"] == j["pairs"], j["why"]
            assert np.abs(g["R"] - tf[:3, :3]).max() <= 1e-6, j["why"]
            assert np.abs(g["t"] - tf[:3, 3] * 1000.0).max() <= 1e-4, j["why"]
            assert np.abs(g["icp_pose"] - np.array(j["icp_pose"])).max() <= 1e-6, j["why"]
        mesh.close()
    finally:
        ctx.close()
