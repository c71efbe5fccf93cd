"""GPU tests of the RGB-D stages (csrc/rgbd.hip, runtime.Rgbd) and the driver (pix2pose_amd.eval_bop_icp):
  * prepare: depth_t, depth_valid and the darkened float32 frame equal tests/rgbd_ref.py bit for bit (u16 and f32 depth, NaN and
    threshold pixels, depth_scale 0.1 and 1.0) at 640x480, 720x540, 1280x960 and 53x37;
  * est_pose on the device frame gives the records est_pose_batch gives on the host-darkened float32 frame;
  * p2p_rgbd_refine equals p2p_refine_depth_batch bit for bit (records and inlier masks); unions of 30 pixels are gated, 31 refined;
  * p2p_rgbd_resolve equals the restatement's walk on random outcome tables (64 images a call, up to 30 rois, obj 1, ties, ratio 0.5);
  * p2p_rgbd_resolve, fed the outcomes of tests/golden/reference_icp3d.json, gives the rows of the reference's own loop;
  * the driver end to end (objects 1 and 2): its rows equal the host chain's (est_pose_batch on host-darkened frames, refine_depth_batch
    per candidate, the restatement's walk), batch_images 1 and 8 agree, refined poses are closer to the truth than the est_pose
    poses, and the CLI writes the CSV."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depth_ref as D  # noqa: E402
import rgbd_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pix2pose_amd.runtime import Context
    c = Context(0, max_batch=16, winograd="always")
    yield c
    c.close()


def raw_frames(rs, H, W, scale, dtype):
    raw = rs.uniform(0, 2.6 / scale * 1000, (H, W)).astype(np.float32)
    edges = []
    for thr in (0.2, 2.2):
        t = np.float32(thr)
        r = np.float32(t / np.float32(scale) * np.float32(1000))
        for _ in range(100):
            r = np.nextafter(r, np.float32(0))
        for _ in range(200):
            edges.append(r)
            r = np.nextafter(r, np.float32(1e9))
    flat = raw.reshape(-1)
    flat[:len(edges)] = edges
    flat[rs.rand(flat.size) < 0.05] = 0
    if dtype == np.uint16:
        raw = np.clip(np.rint(raw), 0, 65535).astype(np.uint16)
        raw.reshape(-1)[:200] = np.arange(1900, 2100) if scale == 0.1 else np.arange(150, 350)
    else:
        flat[rs.rand(flat.size) < 0.02] = np.nan
        flat[5] = np.inf
    return raw


@pytest.mark.parametrize("H,W", [(480, 640), (540, 720), (960, 1280), (37, 53)])
def test_prepare_bit_exact(ctx, H, W):
    from pix2pose_amd.runtime import Rgbd
    rs = np.random.RandomState(H)
    rg = Rgbd(ctx)
    for dtype in (np.uint16, np.float32):
        for scale in (0.1, 1.0):
            raws = [raw_frames(rs, H, W, scale, dtype) for _ in range(2)]
            rgbs = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)]
            rg.load(rgbs, raws, [scale, scale], np.zeros((1, H, W), np.uint8), [1])
            for i in range(2):
                d, v, f = rg.read(i)
                d0, v0, f0 = RR.prepare(raws[i], scale, rgbs[i])
                np.testing.assert_array_equal(d.view(np.uint32), d0.view(np.uint32))
                np.testing.assert_array_equal(v, v0)
                np.testing.assert_array_equal(f.view(np.uint32), f0.view(np.uint32))
                assert v0.any() and (~v0).any()
    rg.close()


def test_est_pose_on_the_device_frame(ctx):
    import torch
    from pix2pose_amd import synthetic, weights as W
    from pix2pose_amd.runtime import Generator, ObjectSpec, Rgbd, est_pose_batch
    sc = synthetic.make_scene(8, seed=5, n_images=2)
    gen = Generator(W.synthetic_weights("resnet50", 1), "resnet50", ctx)
    spec = ObjectSpec(gen, synthetic.OBJ_PARAM, [0.2, 0.3, 0.35], 0.2)
    rs = np.random.RandomState(2)
    H, Wd = sc["images"].shape[1:3]
    raws = [raw_frames(rs, H, Wd, 0.1, np.uint16) for _ in range(2)]
    rg = Rgbd(ctx)
    rg.load(list(sc["images"]), raws, [0.1, 0.1], np.zeros((1, H, Wd), np.uint8), [0])
    host = [RR.prepare(raws[i], 0.1, sc["images"][i])[2] for i in range(2)]
    j1, j2 = torch.from_numpy(sc["inject1"]).cuda(), torch.from_numpy(sc["inject2"]).cuda()
    torch.cuda.synchronize()
    kw = dict(inject1=j1.data_ptr(), inject2=j2.data_ptr(), inject_slots=3)
    a, _ = est_pose_batch(ctx, [spec], [rg.image(0), rg.image(1)], sc["dets"], **kw)
    b, _ = est_pose_batch(ctx, [spec], host, sc["dets"], **kw)
    assert sum(int(p.status) == 0 for p in a) >= 4
    for p, q in zip(a, b):
        assert bytes(p) == bytes(q)
    rg.close()
    gen.close()


# ---------------------------------------------------------------------------------- refine
H, W = 480, 640
K = D.K_640


@pytest.fixture(scope="module")
def mesh(ctx):
    from pix2pose_amd.runtime import Mesh
    v, t = D.l_mesh(8)
    return Mesh(ctx, v, t)


def true_pose(k):
    R = D.rot(0, 20 + 7 * k) @ D.rot(1, -25 + 11 * k) @ D.rot(2, 5 * k)
    t = np.array([-40.0 + 25 * k, 20.0 - 10 * k, 650.0 + 30 * k])
    return R, t


def sensor(ctx, mesh, k, seed):
    from pix2pose_amd import runtime
    R, t = true_pose(k)
    obj = runtime.render_depth_batch(ctx, [mesh], [{"mesh": 0, "camK": K, "R": R, "t": t}], H, W)[0]
    rs = np.random.RandomState(seed)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    wall = (1.1 + 0.05 * np.sin(jj / 31.0) * np.cos(ii / 23.0)).astype(np.float32)
    d = np.where(obj > 0, obj + rs.normal(scale=0.0005, size=obj.shape).astype(np.float32), wall).astype(np.float32)
    d[rs.rand(H, W) < 0.03] = 0
    d[rs.rand(H, W) < 0.01] = np.nan
    return (d * 1000).astype(np.float32), obj > 0        # raw in mm, depth_scale 1.0


def test_refine_equals_refine_depth_batch(ctx, mesh):
    from pix2pose_amd import _lib, runtime
    raws, sil = zip(*[sensor(ctx, mesh, k, 300 + k) for k in range(4)])
    rgbs = [np.full((H, W, 3), 100, np.uint8)] * 4
    rs = np.random.RandomState(7)
    masks, mimg = [], []
    for k in range(4):
        for g in range(3):
            m = sil[k].copy()
            for _ in range(g):
                m[1:] |= m[:-1]; m[:, 1:] |= m[:, :-1]
            masks.append(m); mimg.append(k)
    # exact union sizes 30 and 31 (depth valid everywhere at these pixels), and an empty one
    for n in (30, 31, 0):
        m = np.zeros((H, W), bool)
        ys, xs = np.nonzero(sil[0] & (raws[0] > 300) & (raws[0] < 2100))
        m[ys[:n], xs[:n]] = True
        masks.append(m); mimg.append(0)
    rg = runtime.Rgbd(ctx)
    rg.load(rgbs, list(raws), [1.0] * 4, np.array(masks), mimg)
    jobs, midx = [], []
    for j in range(256):
        k = j % 4
        R, t = true_pose(k)
        R = D.rot(1, rs.uniform(-3, 3)) @ R
        t = t + rs.uniform(-8, 8, 3)
        jobs.append({"image": k, "mesh": 0, "camK": K, "R": R, "t": t})
        midx.append(3 * k + (j // 4) % 3)
    for s, n in enumerate((30, 31, 0)):
        jobs.append({"image": 0, "mesh": 0, "camK": K, "R": true_pose(0)[0], "t": true_pose(0)[1]})
        midx.append(12 + s)
    recs, cnt, inl = rg.refine([mesh], jobs, midx, inlier_masks=True, raw=True)
    assert list(cnt[-3:]) == [30, 31, 0]
    host_d = [RR.prepare(raws[k], 1.0, rgbs[k])[:2] for k in range(4)]
    unions = [np.asarray(masks[m]) & host_d[j["image"]][1] for j, m in zip(jobs, midx)]
    np.testing.assert_array_equal(cnt, [u.sum() for u in unions])
    keep = [j for j in range(len(jobs)) if cnt[j] > 30]
    assert len(keep) == len(jobs) - 2
    hj = [dict(jobs[j], union_mask=unions[j]) for j in keep]
    ref = (_lib.RefineResult * len(hj))()
    from pix2pose_amd.runtime import _depth_jobs, _icp_params
    import ctypes as C
    keepalive = []
    arr = _depth_jobs(hj, keepalive)
    dp = (C.c_void_p * 4)(*[d[0].ctypes.data for d in host_d])
    masks_h = np.zeros((len(hj), H, W), np.uint8)
    p = _icp_params()
    mh = (C.c_void_p * 1)(mesh.handle.value)
    _lib.check(_lib.lib().p2p_refine_depth_batch(ctx.handle, mh, 1, dp, 4, arr, len(hj), H, W, C.byref(p), ref, masks_h.ctypes.data),
               "p2p_refine_depth_batch")
    for i, j in enumerate(keep):
        assert bytes(recs[j]) == bytes(ref[i]), j
        np.testing.assert_array_equal(inl[j], masks_h[i].astype(bool))
    for j in (len(jobs) - 3, len(jobs) - 1):
        assert recs[j].icp.status == _lib.RGBD_SMALL_UNION and recs[j].score.fcn == 0 and not inl[j].any()
        assert list(recs[j].t) == list(jobs[j]["t"])
    assert sum(recs[j].icp.status == 0 for j in keep) > 200
    rg.close()


# ---------------------------------------------------------------------------------- resolve
def test_resolve_equals_restatement(ctx):
    from pix2pose_amd import _lib, runtime
    Hs, Ws = 24, 32
    rs = np.random.RandomState(21)
    for call in range(3):
        imgs = []
        for i in range(64):
            n_t = rs.randint(1, 4)
            targets = [int(x) for x in rs.choice([1, 2, 3, 5], n_t, replace=False)]
            if 1 not in targets and rs.rand() < 0.7:
                targets[0] = 1
            counts = [int(rs.randint(1, 3)) for _ in targets]
            n_r = int(rs.randint(0, 31))
            rois = [[-1, -1, 4, 4] if rs.rand() < 0.05 else [0, 0, 4, 4] for _ in range(n_r)]
            obj_ids = [int(rs.choice(targets + [9])) for _ in range(n_r)]
            scores = [float(rs.choice([0.5, 0.25, rs.rand()])) for _ in range(n_r)]
            base = [rs.rand(Hs, Ws) < 0.3 for _ in range(3)]
            masks = [base[rs.randint(3)] if rs.rand() < 0.6 else rs.rand(Hs, Ws) < 0.3 for _ in range(n_r)]
            if n_r and rs.rand() < 0.2:
                masks[0] = np.zeros((Hs, Ws), bool)
            table = {}
            for rnd in range(2):
                for r in range(n_r):
                    for o in targets:
                        st = rs.choice(["ok"] * 6 + ["est", "near", "union", "refine"])
                        table[(rnd, r, o)] = {"stage": str(st), "R": rs.rand(3, 3), "t": rs.rand(3) * 1000,
                                              "fcn": float(rs.choice([0.0, 8.0, 16.0, rs.rand() * 30])),
                                              "ratio": float(rs.choice([0.5, np.nextafter(0.5, 1), rs.rand()])),
                                              "inlier_mask": masks[r] & (rs.rand(Hs, Ws) < 0.9)}
            imgs.append({"targets": targets, "counts": counts, "rois": rois, "obj_ids": obj_ids, "scores": scores, "masks": masks,
                         "table": table})
        allm, mimg = [], []
        for i, im in enumerate(imgs):
            im["mask0"] = len(allm)
            allm += im["masks"]; mimg += [i] * len(im["masks"])
        rg = runtime.Rgbd(ctx)
        rg.load([np.zeros((Hs, Ws, 3), np.uint8)] * 64, [np.zeros((Hs, Ws), np.uint16)] * 64, [1.0] * 64,
                np.array(allm) if allm else np.zeros((0, Hs, Ws)), mimg)
        roi_used = np.zeros(sum(len(im["rois"]) for im in imgs), np.int32)
        inst_pred = np.zeros(sum(len(im["targets"]) for im in imgs), np.int32)
        got = [[] for _ in imgs]
        for rnd in range(2):
            recs, rmasks, cand = [], [], []
            ro = to = 0
            for i, im in enumerate(imgs):
                nr, nt = len(im["rois"]), len(im["targets"])
                from pix2pose_amd.eval_bop_icp import round0_candidates, round1_candidates
                cs = (round0_candidates(im["targets"], im["rois"], im["obj_ids"]) if rnd == 0 else
                      round1_candidates(im["targets"], im["counts"], im["rois"], roi_used[ro:ro + nr], inst_pred[to:to + nt]))
                per = [[] for _ in range(nr)]
                for r, o in cs:
                    oc = im["table"][(rnd, r, o)]
                    code = {"est": _lib.RGBD_EST_FAILED, "near": _lib.RGBD_NEAR}.get(oc["stage"])
                    if code is None:
                        rec = _lib.RefineResult()
                        rec.icp.status = {"ok": 0, "union": _lib.RGBD_SMALL_UNION, "refine": -1}[oc["stage"]]
                        rec.score.fcn, rec.score.ratio = oc["fcn"], oc["ratio"]
                        rec.R[:] = list(oc["R"].reshape(9)); rec.t[:] = list(oc["t"])
                        code = len(recs)
                        recs.append(rec); rmasks.append(oc["inlier_mask"] if oc["stage"] == "ok" else np.zeros((Hs, Ws), bool))
                    per[r].append((o, code))
                cand.append({"targets": im["targets"], "inst_counts": im["counts"],
                             "rois": [{"obj": im["obj_ids"][r], "score": im["scores"][r], "valid": not (roi[0] == -1 and roi[1] == -1),
                                       "mask": im["mask0"] + r, "cands": per[r]} for r, roi in enumerate(im["rois"])]})
                ro += nr; to += nt
            arr = (_lib.RefineResult * max(len(recs), 1))(*recs)
            rows = rg.resolve(rnd, cand, roi_used, inst_pred, host_records=arr if recs else (_lib.RefineResult * 1)(),
                              host_masks=np.array(rmasks) if rmasks else np.zeros((1, Hs, Ws), bool))
            ro = 0
            for i, im in enumerate(imgs):
                got[i] += [w for w in rows[ro:ro + len(im["rois"])] if w[0] != 0]
                ro += len(im["rois"])
        n_rows = n_r1 = 0
        for i, im in enumerate(imgs):
            want, _ = RR.walk(im["targets"], im["counts"], im["rois"], im["obj_ids"], im["scores"], im["masks"],
                              lambda a, b, c, im=im: im["table"][(a, b, c)], (Hs, Ws))
            assert len(want) == len(got[i]), i
            for w, g in zip(want, got[i]):
                assert (int(g[0]), g[1], int(g[14]), int(g[15])) == (w["obj_id"], w["score"], w["round"], w["r_id"])
                np.testing.assert_array_equal(g[2:11], np.asarray(w["R"]).reshape(9))
                np.testing.assert_array_equal(g[11:14], w["t"])
            n_rows += len(want)
            n_r1 += sum(1 for w in want if w["round"] == 1)
        assert n_rows > 100 and n_r1 > 5
        rg.close()


# ---------------------------------------------------------------------------------- driver end to end
def write_ply(path, v, t):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(t)))
        for p in v:
            f.write("%r %r %r\n" % tuple(float(x) for x in p))
        for q in t:
            f.write("3 %d %d %d\n" % tuple(int(x) for x in q))


def synthetic_dump(ctx, mesh, tmp_path, n_img=6, dets_per_image=3, seed=9):
    """A scene for the driver: decoder maps and true poses from synthetic.make_scene, sensor depth rendered from the L mesh at the true
    poses with holes, detector masks = silhouettes (the first duplicated, so the occupancy skips fire), objects 1 and 2 alternating."""
    from pix2pose_amd import runtime, synthetic
    sc = synthetic.make_scene(dets_per_image * n_img, seed=seed, n_images=n_img)
    v, t = D.l_mesh(8)
    write_ply(str(tmp_path / "obj_000001.ply"), v, t)
    Kc = sc["dets"][0][3]
    by_img = {}
    for k, d in enumerate(sc["dets"]):
        by_img.setdefault(d[0], []).append(k)
    images, targets, key, order, host = [], [], [], [], []
    for i in range(n_img):
        dets = by_img.get(i, [])
        depth = np.full((H, W), 1100.0, np.float32)
        sils = []
        for k in dets:
            R, tt = sc["gt"][k]
            obj = runtime.render_depth_batch(ctx, [mesh], [{"mesh": 0, "camK": Kc, "R": R, "t": tt}], H, W)[0]
            depth = np.where((obj > 0) & (obj * 1000 < depth), obj * 1000, depth).astype(np.float32)
            sils.append(obj > 0)
        rs = np.random.RandomState(i)
        depth[rs.rand(H, W) < 0.02] = 0
        rois = [list(sc["dets"][k][2]) for k in dets]
        masks = list(sils)
        if dets:
            rois.append(rois[0]); masks.append(sils[0]); dets = dets + [dets[0]]
        obj_ids = [1 + (r % 2) for r in range(len(rois))]
        if len(rois) > 1:
            obj_ids[-1] = obj_ids[0]                     # the duplicate names the same object
        np.save(tmp_path / ("rgb%d.npy" % i), sc["images"][i])
        np.save(tmp_path / ("d%d.npy" % i), depth)
        np.save(tmp_path / ("m%d.npy" % i), np.stack(masks, 2) if masks else np.zeros((H, W, 0), bool))
        scores = [0.9 - 0.01 * r for r in range(len(rois))]
        tg = sorted(set(obj_ids)) or [1]
        cnt = [max(1, obj_ids.count(o) - 1) for o in tg]
        images.append({"scene_id": 1, "im_id": i, "rgb": "rgb%d.npy" % i, "depth": "d%d.npy" % i, "depth_scale": 1.0,
                       "cam_K": list(Kc.reshape(9)), "rois": rois, "obj_ids": obj_ids, "scores": scores, "masks": "m%d.npy" % i})
        for o, c in zip(tg, cnt):
            targets.append({"scene_id": 1, "im_id": i, "obj_id": o, "inst_count": c})
        for r, k in enumerate(dets):
            key.append((i, r)); order.append(k)
        host.append({"scene_id": 1, "im_id": i, "gi": i, "rgb": sc["images"][i], "raw": depth, "depth_scale": 1.0, "K": Kc,
                     "targets": tg, "counts": cnt, "rois": rois, "obj_ids": obj_ids, "scores": scores, "masks": masks,
                     "model_ids": [1, 2], "gt": [sc["gt"][k] for k in dets]})
    nf = dict(zip(["x_scale", "y_scale", "z_scale", "x_ct", "y_ct", "z_ct"], synthetic.OBJ_PARAM.tolist()))
    dump = {"im_size": [W, H], "model_ids": [1, 2], "norm_factor": {"1": nf, "2": nf},
            "weights": {"1": "synthetic:resnet50:1", "2": "synthetic:resnet50:1"},
            "meshes": {"1": "obj_000001.ply", "2": "obj_000001.ply"}, "targets": targets, "images": images}
    inject = {"key": np.array(key), "inject1": sc["inject1"][order], "inject2": sc["inject2"][order]}
    return dump, inject, host


CFG = {"backbone": "resnet50", "outlier_th": [0.2, 0.3, 0.35], "inlier_th": 0.2, "score_type": 2, "task_type": 2, "cand_factor": 2,
       "generator_chunk": 64, "skimage": "0.14"}


def test_driver_end_to_end(ctx, mesh, tmp_path):
    from pix2pose_amd import eval_bop_icp as E, runtime, synthetic, weights as Wt
    dump, inject, host = synthetic_dump(ctx, mesh, tmp_path)
    cfg = dict(CFG, path_to_output=str(tmp_path / "out"))
    a = E.run(cfg, "ycbv", dump, base_dir=str(tmp_path), batch_images=1, inject=inject, write_csv=False)
    b = E.run(cfg, "ycbv", dump, base_dir=str(tmp_path), batch_images=8, inject=inject, write_csv=False)
    # the host chain: est_pose_batch on host-darkened frames, refine_depth_batch per candidate, the restatement's walk
    gen = runtime.Generator(Wt.synthetic_weights("resnet50", 1), "resnet50", ctx)
    spec = runtime.ObjectSpec(gen, synthetic.OBJ_PARAM, CFG["outlier_th"], CFG["inlier_th"])
    m2 = runtime.Mesh(ctx, *D.l_mesh(8))
    inj = dict(inject, row={(int(i), int(r)): k for k, (i, r) in enumerate(inject["key"])})
    c, evaluated = RR.host_chain(ctx, [spec, spec], [mesh, m2], host, task_type=2, inject=inj, anti_aliasing="0.14")
    assert len(a) >= 6 and len(a) == len(b) == len(c)
    assert {r["obj_id"] for r in a} == {1, 2}
    for x, y, z in zip(a, b, c):
        for q in (y, z):
            assert (x["scene_id"], x["im_id"], x["obj_id"], x["score"]) == (q["scene_id"], q["im_id"], q["obj_id"], q["score"])
            np.testing.assert_array_equal(np.asarray(x["R"]).reshape(-1), np.asarray(q["R"]).reshape(-1))
            np.testing.assert_array_equal(np.asarray(x["t"]).reshape(-1), np.asarray(q["t"]).reshape(-1))
    # refined poses are closer to the truth than the est_pose poses
    e_est, e_ref = [], []
    for im, ev, cache in evaluated:
        for (r, o), oc in cache.items():
            if oc["stage"] == "ok":
                Rg, tg = im["gt"][r]
                e_est.append(np.linalg.norm(oc["t_est"] - tg)); e_ref.append(np.linalg.norm(oc["t"] - tg))
    assert len(e_ref) >= 6 and np.median(e_ref) < np.median(e_est), (np.median(e_ref), np.median(e_est))
    # the CLI writes the CSV
    json.dump(dump, open(tmp_path / "dump.json", "w"))
    cfg_fn = tmp_path / "cfg.json"
    json.dump(dict(cfg, batch_images=4), open(cfg_fn, "w"))
    np.savez(tmp_path / "inject.npz", **inject)
    env = dict(os.environ, P2P_EVAL_INJECT=str(tmp_path / "inject.npz"))
    root = os.path.dirname(HERE)
    subprocess.run([sys.executable, "-m", "pix2pose_amd.eval_bop_icp", "0", str(cfg_fn), "ycbv", str(tmp_path / "dump.json")], cwd=root,
                   env=env, check=True, timeout=600)
    lines = open(tmp_path / "out" / E.output_name("ycbv")).read().splitlines()
    assert lines[0] == "scene_id,im_id,obj_id,score,R,t,time" and len(lines) == len(a) + 1


def test_resolve_reproduces_the_reference_fixture(ctx):
    """The resolve kernel, fed the outcomes of tests/golden/reference_icp3d.json through the host-record argument, gives the rows the
    reference's own loop gave.  The fixture holds an IoU of exactly 7/10 and a round-1 roi whose skip is decided by the last scored
    candidate's mask, so `>=` at 0.7 and the best candidate's mask fail here."""
    import test_rgbd_golden_cpu as GC
    from golden.make_reference_normals_vectors import b64_f32, b64_u8
    from pix2pose_amd import _lib, runtime
    from pix2pose_amd.eval_bop import rank_image_results
    from pix2pose_amd.eval_bop_icp import round0_candidates, round1_candidates
    G = GC.load()
    Hs, Ws = G["H"], G["W"]
    raw = b64_f32(G["raw_depth"], (Hs, Ws))
    depth_t, depth_valid, _ = RR.prepare(raw, G["depth_scale"], np.zeros((Hs, Ws, 3), np.uint8))
    ims = G["images"]
    allm, mimg = [], []
    for i, im in enumerate(ims):
        im["mask0"] = len(allm)
        im["mk"] = [b64_u8(m, (Hs, Ws)).astype(bool) for m in im["masks"]]
        allm += im["mk"]; mimg += [i] * len(im["mk"])
    rg = runtime.Rgbd(ctx)
    rg.load([np.zeros((Hs, Ws, 3), np.uint8)] * len(ims), [raw] * len(ims), [G["depth_scale"]] * len(ims), np.array(allm), mimg)
    roi_used = np.zeros(sum(len(im["rois"]) for im in ims), np.int32)
    inst_pred = np.zeros(sum(len(im["targets"]) for im in ims), np.int32)
    got = [[] for _ in ims]
    for rnd in range(2):
        recs, rmasks, cand = [], [], []
        ro = to = 0
        for im in ims:
            nr, nt = len(im["rois"]), len(im["targets"])
            table = {(o["r_id"], o["obj_id"]): o for o in im["outcomes"]}
            cs = (round0_candidates(im["targets"], im["rois"], im["obj_ids"]) if rnd == 0 else
                  round1_candidates(im["targets"], im["counts"], im["rois"], roi_used[ro:ro + nr], inst_pred[to:to + nt]))
            per = [[] for _ in range(nr)]
            for r, o in cs:
                oc = table.get((r, o))
                union = im["mk"][r] & depth_valid
                if oc is None or (oc["est"] == "ok" and oc["t_est"][2] >= 200 and union.sum() > 30 and oc["icp"] == "ok"
                                  and "render" not in oc):
                    code = _lib.RGBD_NOT_EVALUATED          # the reference never reached it: reaching it is an error
                elif oc["est"] == "fail":
                    code = _lib.RGBD_EST_FAILED
                elif oc["t_est"][2] / 1000 < 0.2:
                    code = _lib.RGBD_NEAR
                else:
                    rec = _lib.RefineResult()
                    inl = np.zeros((Hs, Ws), bool)
                    if union.sum() <= 30:
                        rec.icp.status = _lib.RGBD_SMALL_UNION
                    elif oc["icp"] == "fail":
                        rec.icp.status = -1
                    else:
                        tf = np.array(oc["tf"])
                        sc, inl = D.depth_score(b64_f32(oc["render"], (Hs, Ws)), depth_t, union)
                        rec.score.fcn, rec.score.ratio = sc["fcn"], sc["ratio"]
                        rec.R[:] = list(tf[:3, :3].reshape(9)); rec.t[:] = list(tf[:3, 3] * 1000)
                    code = len(recs)
                    recs.append(rec); rmasks.append(inl)
                per[r].append((o, code))
            cand.append({"targets": im["targets"], "inst_counts": im["counts"],
                         "rois": [{"obj": im["obj_ids"][r], "score": im["scores"][r], "valid": not (roi[0] == -1 and roi[1] == -1),
                                   "mask": im["mask0"] + r, "cands": per[r]} for r, roi in enumerate(im["rois"])]})
            ro += nr; to += nt
        arr = (_lib.RefineResult * max(len(recs), 1))(*recs)
        rows = rg.resolve(rnd, cand, roi_used, inst_pred, host_records=arr,
                          host_masks=np.array(rmasks) if rmasks else np.zeros((1, Hs, Ws), bool))
        ro = 0
        for i, im in enumerate(ims):
            got[i] += [{"obj_id": int(w[0]), "score": w[1], "R": w[2:11].copy(), "t": w[11:14].copy()}
                       for w in rows[ro:ro + len(im["rois"])] if w[0] != 0]
            ro += len(im["rois"])
    out = []
    for i, im in enumerate(ims):
        out += rank_image_results(got[i], im["targets"], im["counts"], '2', im["scene_id"], im["im_id"], 0.0)
    assert len(out) == len(G["rows"])
    for a, b in zip(out, G["rows"]):
        assert (a["scene_id"], a["im_id"], a["obj_id"]) == (b["scene_id"], b["im_id"], b["obj_id"])
        assert abs(a["score"] - b["score"]) <= 1e-12 * abs(b["score"])
        np.testing.assert_array_equal(np.asarray(a["R"]).reshape(-1), b["R"])
        np.testing.assert_array_equal(np.asarray(a["t"]).reshape(-1), b["t"])
    rg.close()
