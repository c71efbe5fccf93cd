"""CPU tests of the RGB-D restatement (tests/rgbd_ref.py): the frame-preparation rules of tools/5_evaluation_bop_icp3d.py :360-370,
and the walk of :394-510 over the candidate superset the batched driver evaluates (pix2pose_amd.eval_bop_icp) against the walk
that evaluates each candidate on demand."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rgbd_ref as RR  # noqa: E402


def f32_prepare(raw, scale, rgb):
    """The rules written out with float32 scalars, element by element (an independent statement of :360-370)."""
    raw = np.asarray(raw)
    H, W = raw.shape
    d = np.zeros((H, W), np.float32)
    v = np.zeros((H, W), bool)
    f = np.asarray(rgb).astype(np.float32).copy()
    s = np.float32(scale)
    for i in range(H):
        for j in range(W):
            x = np.float32(np.float32(raw[i, j]) / np.float32(1000)) * s
            d[i, j] = x
            v[i, j] = bool(x > np.float32(0.2)) and bool(x < np.float32(2.2))
            keep = v[i, j] or np.isnan(x) or x == 0
            if not keep:
                f[i, j] = f[i, j] * np.float32(0.1)
    return d, v, f


def edge_depths(scale):
    """Raw values whose depth_t lands one float32 ulp below, on and above float32(0.2) and float32(2.2), plus NaN, 0 and inf."""
    vals = []
    s = np.float32(scale)
    for thr in (0.2, 2.2):
        t = np.float32(thr)
        want = {np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(10))}
        r = np.float32(t / s * np.float32(1000))
        for _ in range(200):
            r = np.nextafter(r, np.float32(0))
        for _ in range(400):
            if np.float32(r / np.float32(1000)) * s in want:
                vals.append(r)
            r = np.nextafter(r, np.float32(1e9))
    return np.array(vals + [np.nan, 0.0, -0.0, np.inf, 199.99, 2200.0, 1500.0], np.float32)


def test_prepare_thresholds_nan_and_scales():
    rs = np.random.RandomState(0)
    for scale in (0.1, 1.0):
        raw = edge_depths(scale)
        raw = np.concatenate([raw, rs.uniform(0, 30000 if scale == 0.1 else 3000, 64 - raw.size % 64).astype(np.float32)]).reshape(4, -1)
        rgb = rs.randint(0, 256, raw.shape + (3,)).astype(np.uint8)
        d, v, f = RR.prepare(raw, scale, rgb)
        d2, v2, f2 = f32_prepare(raw, scale, rgb)
        np.testing.assert_array_equal(d.view(np.uint32), d2.view(np.uint32))
        np.testing.assert_array_equal(v, v2)
        np.testing.assert_array_equal(f.view(np.uint32), f2.view(np.uint32))
        # the float32 comparison, not float64: a depth of float32(0.2) is not valid although float(float32(0.2)) > 0.2
        assert float(np.float32(0.2)) > 0.2
        for thr in (0.2, 2.2):
            t = np.float32(thr)
            assert (d == t).any() and not v[d == t].any()
            assert ((d == np.nextafter(t, np.float32(0))) | (d == np.nextafter(t, np.float32(10)))).any()
        assert v[d == np.nextafter(np.float32(0.2), np.float32(10))].all() and v[d == np.nextafter(np.float32(2.2), np.float32(0))].all()
        assert v[(d > np.float32(0.2)) & (d < np.float32(2.2))].all()
        nan = np.isnan(d)
        assert nan.any() and not v[nan].any()
        np.testing.assert_array_equal(f[nan], rgb[nan].astype(np.float32))          # NaN: not darkened
        inf = np.isinf(d)
        np.testing.assert_array_equal(f[inf], np.float32(0.1) * rgb[inf].astype(np.float32))


def test_prepare_float64_thresholds_differ():
    """The mutation "float64 thresholds" changes depth_valid at the edge pixels."""
    raw = edge_depths(1.0)
    d, v, _ = RR.prepare(raw[None], 1.0, np.zeros((1, raw.size, 3), np.uint8))
    with np.errstate(invalid="ignore"):
        v64 = (d.astype(np.float64) > 0.2) & (d.astype(np.float64) < 2.2)
    assert (v64 != v).any()


def test_prepare_u16_equals_f32_input():
    rs = np.random.RandomState(3)
    raw = rs.randint(0, 65536, (37, 53)).astype(np.uint16)
    rgb = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    for scale in (0.1, 1.0):
        a = RR.prepare(raw, scale, rgb)
        b = RR.prepare(raw.astype(np.float32), scale, rgb)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


def random_image(rs, H=12, W=16):
    """One image of a random outcome table: targets (obj 1 often among them), rois, masks that overlap, and per (round, roi, obj)
    outcomes with ties, ratio exactly 0.5 and every failure stage."""
    n_t = rs.randint(1, 4)
    targets = list(rs.choice([1, 2, 3, 5, 7], n_t, replace=False))
    if rs.rand() < 0.6 and 1 not in targets:
        targets[0] = 1
    counts = [int(rs.randint(1, 3)) for _ in targets]
    n_r = rs.randint(0, 9)
    rois = [[-1, -1, 5, 5] if rs.rand() < 0.1 else [1, 1, 8, 8] for _ in range(n_r)]
    obj_ids = [int(rs.choice(targets + [9])) for _ in range(n_r)]
    scores = [float(rs.choice([0.5, 0.9, rs.rand()])) for _ in range(n_r)]
    base = [rs.rand(H, W) < 0.3 for _ in range(3)]
    masks = [base[rs.randint(3)] if rs.rand() < 0.5 else rs.rand(H, W) < 0.3 for _ in range(n_r)]
    if n_r and rs.rand() < 0.2:
        masks[0] = np.zeros((H, W), bool)
    table = {}
    for rnd in range(2):
        for r in range(n_r):
            for o in set(targets):
                st = rs.choice(["ok"] * 5 + ["est", "near", "union", "refine"])
                R = np.eye(3) * rs.rand()
                t = rs.rand(3) * 1000
                table[(rnd, r, o)] = {"stage": st, "R": R, "t": t, "fcn": float(rs.choice([0.0, 10.0, 20.0, rs.rand() * 30])),
                                      "ratio": float(rs.choice([0.5, np.nextafter(0.5, 1), rs.rand()])),
                                      "inlier_mask": masks[r] & (rs.rand(H, W) < 0.9) if n_r else None}
    return {"targets": targets, "counts": counts, "rois": rois, "obj_ids": obj_ids, "scores": scores, "masks": masks, "table": table,
            "shape": (H, W)}


def walk_on_demand(im):
    return RR.walk(im["targets"], im["counts"], im["rois"], im["obj_ids"], im["scores"], im["masks"], lambda a, b, c: im["table"][(a, b, c)],
                   im["shape"])


def walk_from_superset(im):
    """Evaluate the driver's superset first (round 0 from the dump; round 1 after round 0), then walk reading only those."""
    from pix2pose_amd import eval_bop_icp as E
    c0 = set((0, r, o) for r, o in E.round0_candidates(im["targets"], im["rois"], im["obj_ids"]))
    done = {k: im["table"][k] for k in c0}

    def outcome(rnd, r, o):
        assert (rnd, r, o) in done, "the walk reached a candidate outside the evaluated superset"
        return done[(rnd, r, o)]
    rows0, _ = RR.walk(im["targets"], im["counts"], im["rois"], im["obj_ids"], im["scores"], im["masks"],
                       lambda a, b, c: outcome(a, b, c) if a == 0 else {"stage": "est"}, im["shape"])
    used, pred = RR.state_after_round0(im["targets"], im["counts"], rows0)
    used_flags = [r in used for r in range(len(im["rois"]))]
    for r, o in E.round1_candidates(im["targets"], im["counts"], im["rois"], used_flags, pred):
        done[(1, r, o)] = im["table"][(1, r, o)]
    return RR.walk(im["targets"], im["counts"], im["rois"], im["obj_ids"], im["scores"], im["masks"], outcome, im["shape"])


def test_superset_resolution_equals_on_demand_walk():
    rs = np.random.RandomState(11)
    n_rows = n_r1 = 0
    for _ in range(300):
        im = random_image(rs)
        a, ea = walk_on_demand(im)
        b, eb = walk_from_superset(im)
        assert ea == eb
        assert [(r["obj_id"], r["score"], r["round"], r["r_id"]) for r in a] == [(r["obj_id"], r["score"], r["round"], r["r_id"]) for r in b]
        n_rows += len(a)
        n_r1 += sum(1 for r in a if r["round"] == 1)
    assert n_rows > 300 and n_r1 > 20


def test_walk_quirks():
    """The bool occupancy (obj 1 skipped by its own earlier roi in round 0, obj 2 not), NaN IoU, the last-scored mask update,
    ratio exactly 0.5 and the round-1 break, on a hand-made image."""
    H, W = 4, 8
    m = np.zeros((H, W), bool); m[:, :4] = True
    empty = np.zeros((H, W), bool)
    rois = [[0, 0, 4, 4]] * 5
    ok = lambda fcn, ratio, mask: {"stage": "ok", "R": np.eye(3), "t": np.zeros(3), "fcn": fcn, "ratio": ratio, "inlier_mask": mask}  # noqa: E731
    # round 0: roi 0 obj 1 fills the occupancy with m; roi 1 obj 1 same mask -> IoU 1 > 0.7: skipped; roi 2 obj 2 same mask: not
    # skipped (occupancy == 2 is empty); roi 3 an empty mask (NaN IoU: not skipped)
    table = {(0, 0, 1): ok(10.0, 0.9, m), (0, 2, 2): ok(10.0, 0.9, m), (0, 3, 2): ok(5.0, 0.9, empty)}
    rows, ev = RR.walk([1, 2], [1, 5], rois[:4], [1, 1, 2, 2], [1.0] * 4, [m, m, m, empty], lambda a, b, c: table[(a, b, c)], (H, W))
    assert (0, 1, 1) not in ev and (0, 2, 2) in ev and (0, 3, 2) in ev
    # round 1: roi 1 is used by none; occupancy != 0 is m: roi 1 (mask m) IoU 1 -> skipped; the missing set {2} stays
    assert [(r["round"], r["r_id"]) for r in rows] == [(0, 0), (0, 2), (0, 3)]
    # last-scored mask: two candidates, the first is best, the second (lower score) scores last and its mask is the update
    a = np.zeros((H, W), bool); a[0, 6] = True
    b = np.zeros((H, W), bool); b[3, 7] = True
    tb = {(1, 0, 1): ok(20.0, 0.9, a), (1, 0, 2): ok(10.0, 0.9, b), (1, 1, 2): ok(10.0, 0.5, a), (1, 1, 1): ok(1.0, 0.5, a)}
    tb.update({(0, 0, 9): None})
    mb = np.zeros((H, W), bool); mb[3, 7] = True
    rows, ev = RR.walk([1, 2], [1, 1], [[0, 0, 1, 1], [0, 0, 1, 1]], [9, 9], [1.0, 1.0], [empty, mb],
                       lambda x, y, z: tb[(x, y, z)], (H, W))
    assert rows[0]["obj_id"] == 1 and rows[0]["round"] == 1
    # roi 0 updated the occupancy with b (the last scored), so roi 1 (mask b) has IoU 1 and is skipped
    assert (1, 1, 2) not in ev and len(rows) == 1
