"""The per-pixel glue kernels around the two generator passes (stage1_input / stage1_stats / stage2_input / cand_range / cand_corr)
against the numpy oracle, through the debug taps of est_pose_batch(..., debug=True).

Batches of more than 16 detections of 128-px stage-1 crops take the kernels' shared-work forms (stage1_input: four pixels per thread;
stage2_input: the slots of a detection in one thread); smaller batches and every other crop side take the per-pixel forms, and every
batch builds its correspondences over pixel segments and compacts them in a second launch.  All are held to the same standard: the
float32 network inputs x1 / x2 and every integer (stage-2 boxes, mask counts, candidate records, correspondence counts, inlier counts,
masks, truncated images) are EXACTLY the oracle's; the poses, which follow from the correspondences, within the 1e-6 mm / 1e-4 deg of
the pipeline's own parity test."""
import numpy as np
import pytest

from pix2pose_amd import weights as W
from pix2pose_amd import synthetic as synth

pytestmark = pytest.mark.gpu

TH_O = [0.2, 0.3, 0.35]
TH_I = 0.2


@pytest.fixture(scope="module")
def rig():
    from pix2pose_amd.runtime import Context, Generator, ObjectSpec
    ctx = Context(0, max_batch=64, winograd="off")
    gen = Generator(W.synthetic_weights("paper", 1), "paper", ctx)
    return ctx, ObjectSpec(gen, synth.OBJ_PARAM, TH_O, TH_I)


def _check(rig, sc, min_ok):
    """-> (poses, extras).  Every detection of the scene against the oracle."""
    import torch
    from oracle import est_pose_oracle as E
    from pix2pose_amd.runtime import est_pose_batch
    ctx, spec = rig
    j1 = torch.from_numpy(sc["inject1"]).cuda()
    j2 = torch.from_numpy(sc["inject2"]).cuda()
    torch.cuda.synchronize()
    poses, ex = est_pose_batch(ctx, [spec], list(sc["images"]), sc["dets"], inject1=j1.data_ptr(), inject2=j2.data_ptr(),
                               inject_slots=3, want_masks=True, debug=True)
    n_ok = 0
    for i, p in enumerate(poses):
        def predict(x, stage, slots=None, i=i):
            m = sc["inject1"][i][None] if stage == 1 else sc["inject2"][i][slots]
            return [m[..., :3].copy(), m[..., 3:].copy()]
        img_i, _, bbox, K = sc["dets"][i]
        dbg = {}
        ref = E.est_pose(sc["images"][img_i], bbox, predict, K, sc["obj_param"], TH_O, TH_I, debug=dbg)
        ok_ref = not (isinstance(ref[4], int) and ref[4] == -1)
        assert (p.status == 0) == ok_ref, (i, p.status)
        np.testing.assert_array_equal(np.array(list(p.bbox_t)), ref[5])
        # stage-1 input and statistics
        if "x1" in dbg:
            np.testing.assert_array_equal(ex["x1"][i], dbg["x1"], err_msg="x1 of detection %d" % i)
        if "n_init_mask" in dbg:
            assert p.n_init_mask == dbg["n_init_mask"], i
        slots = dbg.get("slots", [])
        assert p.n_candidates == len(slots), i
        for slot in range(len(TH_O)):      # valid2 of every slot, dropped ones included
            assert ex["cand"][i, slot, 0] == (1 if slot in slots else 0), (i, slot)
        if dbg.get("boxes2"):
            np.testing.assert_array_equal(ex["boxes2"][i], dbg["boxes2"][0])
        # stage-2 inputs and candidate records
        for c, slot in enumerate(slots):
            np.testing.assert_array_equal(ex["x2"][i, slot], dbg["x2"][c], err_msg="x2 of detection %d slot %d" % (i, slot))
            cd = dbg["cands"][c]
            assert ex["cand"][i, slot, 1] == cd["n_non_gray"], (i, slot)
            if cd.get("n_valid", -1) >= 0:
                assert ex["cand"][i, slot, 2] == cd["n_valid"], (i, slot)
            if "n_inliers" in cd:
                assert ex["cand"][i, slot, 3] == cd["n_inliers"], (i, slot)
        for slot in range(len(TH_O)):
            if slot not in slots:
                assert not ex["x2"][i, slot].any(), (i, slot)      # a dropped slot's network input is all zero
        if ok_ref:
            n_ok += 1
            dt, dr = synth.pose_error(ref[2], ref[3], np.array(p.R).reshape(3, 3), np.array(p.t))
            assert dt < 1e-6 and dr < 1e-4, (i, dt, dr)
            assert p.best_slot == slots[dbg["best"]]
            # the selected candidate's correspondences, pixel for pixel: valid mask and truncated uint8 image
            v1, v2, u1, u2 = ref[5]
            H, Wd = ref[1].shape
            np.testing.assert_array_equal(ex["valid_mask"][i][:H * Wd].reshape(H, Wd).astype(bool), ref[1])
            np.testing.assert_array_equal(ex["img_pred"][i][:(v2 - v1) * (u2 - u1) * 3].reshape(v2 - v1, u2 - u1, 3), ref[0])
    assert n_ok >= min_ok, n_ok
    return poses, ex


def test_identity_crops_batch_of_40(rig):
    """(a) 128-px crops, more than a handful: the shared-work forms."""
    _check(rig, synth.make_scene(40, seed=11), 36)


def test_general_crop_sides_40_to_300(rig):
    """(b) every resize is a real resampling: the per-pixel forms, in a batch of more than a handful."""
    _check(rig, synth.make_scene(24, seed=12, bbox_side=(40, 300)), 18)


def test_mixed_batch_stays_on_the_per_pixel_forms(rig):
    """128-px crops and other sides in one batch."""
    a, b = synth.make_scene(14, seed=13), synth.make_scene(10, seed=13, bbox_side=(60, 200))
    sc = {"images": a["images"], "dets": a["dets"] + [(d[0], d[1], d[2], d[3]) for d in b["dets"]], "obj_param": a["obj_param"],
          "inject1": np.concatenate([a["inject1"], b["inject1"]]), "inject2": np.concatenate([a["inject2"], b["inject2"]])}
    _check(rig, sc, 0)


def _move_to_border(sc, idx, dv, du):
    """Shift detection idx's box so that its 128-px square crosses the frame border (the injected maps stay: parity, not pose quality)."""
    img, obj, bbox, K = sc["dets"][idx]
    H, Wd = sc["images"].shape[1:3]
    v = -30 - bbox[0] if dv < 0 else (H - 55 - bbox[0] if dv > 0 else 0)
    u = -30 - bbox[1] if du < 0 else (Wd - 55 - bbox[1] if du > 0 else 0)
    sc["dets"][idx] = (img, obj, [bbox[0] + v, bbox[1] + u, bbox[2] + v, bbox[3] + u], K)


def test_crops_clipped_by_the_frame_border(rig):
    """(c) 128-px squares that leave the frame at the top / left / bottom / right / a corner, inside a batch on the shared-work forms."""
    sc = synth.make_scene(30, seed=14)
    for idx, (dv, du) in enumerate([(-1, 0), (0, -1), (1, 0), (0, 1), (-1, -1), (1, 1)]):
        _move_to_border(sc, 3 * idx, dv, du)
    _, ex = _check(rig, sc, 20)
    b = ex["boxes2"]
    assert any(tuple(b[i, :4]) != tuple(b[i, 4:8]) for i in range(0, 18, 3)), "no stage-2 box was clipped"


def test_slot_without_candidate(rig):
    """(d) valid2 == 0 for one slot (fewer than 10 kept pixels under the first threshold), the other two slots built."""
    sc = synth.make_scene(20, seed=15)
    for i in (2, 9):
        sc["inject1"][i, :, :, 3] = np.maximum(sc["inject1"][i, :, :, 3], np.float32(0.25))      # nothing below th_o[0] = 0.2
    _, ex = _check(rig, sc, 0)
    for i in (2, 9):
        assert ex["cand"][i, 0, 0] == 0 and ex["cand"][i, 1, 0] == 1 and ex["cand"][i, 2, 0] == 1, ex["cand"][i, :, 0]


@pytest.mark.parametrize("n", [1, 3, 257])
def test_batch_sizes(rig, n):
    """(e) one detection, three, and 257: the split of a detection over workgroups and the remainder of the grid."""
    _check(rig, synth.make_scene(n, seed=20 + n), n - n // 8)
