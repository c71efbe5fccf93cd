"""CPU tests of the RGB-D driver's host side (pix2pose_amd.eval_bop_icp, bop_dataset.build_dump(with_depth=True)): the config refusals,
the dump keys, and the depth loader."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def test_config_refusals(monkeypatch):
    from pix2pose_amd import eval_bop_icp as E
    with pytest.raises(ValueError, match="score_type"):
        E.check_config({"score_type": 1})
    with pytest.raises(ValueError, match="detection_pipeline"):
        E.check_config({"score_type": 2}, "retinanet")
    E.check_config({"score_type": 2}, "rcnn")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        E.check_world()
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        E.main(["x", "0", "cfg.json", "ycbv"])
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        E.run({"score_type": 2}, "ycbv", {})
    monkeypatch.setenv("WORLD_SIZE", "1")
    E.check_world()


def test_missing_mask_is_refused():
    from pix2pose_amd import eval_bop_icp as E
    im = {"scene_id": 1, "im_id": 2, "rois": [[0, 0, 4, 4]], "segmentations": [None]}
    with pytest.raises(ValueError, match="detector mask for every detection"):
        E.image_masks(im, ".", 1, (4, 4))


def test_build_dump_with_depth(tmp_path):
    from test_bop_dataset import make_bop_dir
    from pix2pose_amd import bop_dataset as B
    root = str(tmp_path)
    cfg, targets, paths = make_bop_dir(root, "ycbv", weights=False)
    for m in (1, 4):      # the reference keeps the ids whose mesh exists (tools/bop_io.py:129-131)
        open(os.path.join(root, "ycbv", "models", "obj_%06d.ply" % m), "w").close()
    cfg["target_obj"] = [1, 4]
    for m in (1, 4):
        wdir = os.path.join(root, "ycbv", "pix2pose_weights", "%02d" % m)
        os.makedirs(wdir, exist_ok=True)
        open(os.path.join(wdir, "inference.npz"), "w").close()
    dets = [{"scene_id": 48, "image_id": 1, "category_id": 4, "bbox": [200, 100, 60, 80], "score": 0.9}]
    plain = B.build_dump(cfg, "ycbv", dets)
    assert plain == B.build_dump(cfg, "ycbv", dets, with_depth=False)
    assert "meshes" not in plain and all("depth" not in im and "depth_scale" not in im for im in plain["images"])
    d = B.build_dump(cfg, "ycbv", dets, with_depth=True)
    assert set(d) == set(plain) | {"meshes"}
    assert d["meshes"] == {"1": os.path.join(root, "ycbv", "models", "obj_000001.ply"),
                           "4": os.path.join(root, "ycbv", "models", "obj_000004.ply")}
    for a, b in zip(plain["images"], d["images"]):
        extra = {k: v for k, v in b.items() if k not in a}
        assert set(extra) == {"depth", "depth_scale"} and all(a[k] == b[k] for k in a)
        assert b["depth"] == os.path.join(root, "ycbv", "test", "%06d" % b["scene_id"], "depth", "%06d.png" % b["im_id"])
        assert b["depth_scale"] == 0.1
    json.dumps(d)


def test_load_depth(tmp_path):
    from PIL import Image
    from pix2pose_amd import eval_bop_icp as E
    a = (np.arange(12 * 10).reshape(12, 10) * 500).astype(np.uint16)
    fn = str(tmp_path / "d.png")
    Image.fromarray(a).save(fn)
    b = E.load_depth(fn)
    assert b.dtype == np.uint16
    np.testing.assert_array_equal(b, a)
    np.save(tmp_path / "d.npy", a.astype(np.float32) + 0.5)
    c = E.load_depth(str(tmp_path / "d.npy"))
    assert c.dtype == np.float32 and c[0, 0] == 0.5


def test_candidate_sets():
    from pix2pose_amd import eval_bop_icp as E
    rois = [[0, 0, 1, 1], [-1, -1, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1]]
    assert E.round0_candidates([1, 5], rois, [5, 1, 9, 1]) == [(0, 5), (3, 1)]
    assert E.round1_candidates([1, 5], [2, 1], rois, [1, 0, 0, 0], [1, 1]) == [(2, 1), (3, 1)]
    assert E.round1_candidates([1, 5], [1, 1], rois, [0, 0, 0, 0], [1, 1]) == []
