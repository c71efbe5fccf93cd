"""The refinement chain as this library restates it -- tests/normals_ref.py icp_inputs, tests/icp_ref.py icp and refined_pose --
against tests/golden/reference_refine.json, which holds what the reference's own icp_refinement returned with the same ICP and
rasteriser restatements stubbed in (tests/golden/make_reference_refine_vectors.py).  This pins the composition
tf = pose . [R | t_adjusted / 1000] and its units independently of the library's reading of those lines.

Bars: R within 1e-6, t within 1e-4 mm; iteration and pair counts exact.  Measured 1.6e-7 / 6.6e-6 mm: the restated point sets agree
with the reference's getXYZ / get_normal to about 3e-8 relative (tests/golden/reference_normals.json), which moves the ICP's pose by
that much.  The wrong composition order ([R | t] . pose) is off by 6e-3 in R and 7-63 mm in t on these jobs."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_ref as D  # noqa: E402
import icp_ref as I  # noqa: E402
import normals_ref as N  # noqa: E402
from golden.make_reference_normals_vectors import b64_f32, b64_u8  # noqa: E402


def test_restated_chain_reproduces_the_reference_tf():
    G = json.load(open(os.path.join(HERE, "golden", "reference_refine.json")))
    H, W, K = G["H"], G["W"], np.array(G["K"])
    d = b64_f32(G["image"], (H, W))
    mv, mt = np.array(G["mesh_verts"]), np.array(G["mesh_tris"])
    sp = N.scene_points(d, K)
    assert G["params"] == dict(max_iterations=100, tolerance=0.005, rejection_scale=2.5, num_levels=2)
    n_ok = 0
    for j in G["jobs"]:
        R = np.array(j["R"])
        rec = N.icp_inputs(sp, b64_u8(j["union_mask"], (H, W)), np.array(j["t"]), K, lambda t: D.render_depth(mv, mt, K, R, t, H, W))
        assert (rec["status"] != 0) == (j["status"] == -1), j["why"]
        if j["status"] == -1:
            continue
        r = I.icp(rec["src"], rec["tgt"])
        assert r["iterations"] == j["iterations"] and r["pairs"] == j["pairs"], j["why"]
        Rr, tr = I.refined_pose(r["pose"], R, rec["t_adjusted"])
        tf = np.array(j["tf"])
        assert np.abs(Rr - tf[:3, :3]).max() <= 1e-6, j["why"]
        assert np.abs(tr - tf[:3, 3] * 1000.0).max() <= 1e-4, j["why"]
        n_ok += 1
    assert n_ok == 4
