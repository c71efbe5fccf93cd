"""bench.py --dump-outputs: what the writer puts on disk (names, dtypes, the 64 MB budget, the fixed mask sample)."""
import os

import numpy as np

import bench
from pix2pose_amd import _lib
from pix2pose_amd.parallel import poses_to_records


def _poses(n):
    poses = [_lib.Pose() for _ in range(n)]
    for i, p in enumerate(poses):
        p.R[0] = p.R[4] = p.R[8] = 1.0
        p.t[2] = 500.0 + i
        p.frac_inlier = i / n
        p.n_inliers, p.status, p.bbox_t[3] = 3 * i, 0 if i % 5 else -1, 128
    return poses


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_pose_fields_and_records_whole(tmp_path):
    poses = _poses(16)
    rec = poses_to_records(poses)
    bench.dump_outputs(str(tmp_path), poses, rec, None)
    got = _load(str(tmp_path))
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["pose_R"].shape == (16, 3, 3) and np.array_equal(got["pose_t"][:, 2], 500.0 + np.arange(16))
    assert np.array_equal(got["pose_status"], [0 if i % 5 else -1 for i in range(16)])
    assert np.array_equal(got["pose_n_inliers"], 3 * np.arange(16)) and np.array_equal(got["pose_records"], rec)
    assert "valid_mask" not in got and "img_pred" not in got


def test_dump_samples_large_masks_within_budget_and_repeatably(tmp_path):
    poses = _poses(256)
    rec = poses_to_records(poses)
    rs = np.random.RandomState(3)
    extras = {"valid_mask": rs.randint(0, 2, (256, 480 * 640)).astype(np.uint8),
              "img_pred": rs.randint(0, 256, (256, 3 * 128 * 128)).astype(np.uint8)}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, poses, rec, extras)
    bench.dump_outputs(b, poses, rec, extras)
    total = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert total <= bench.DUMP_MAX_BYTES
    ga, gb = _load(a), _load(b)
    assert set(ga) == set(gb) and all(np.array_equal(ga[k], gb[k]) for k in ga)
    for k in ("valid_mask", "img_pred"):
        assert ga[k].dtype == np.float32 and 0 < ga[k].size < extras[k].size
    # small masks go out whole
    small = {k: v[:2, :1000] for k, v in extras.items()}
    bench.dump_outputs(str(tmp_path / "c"), poses[:2], rec[:2], small)
    gc = _load(str(tmp_path / "c"))
    assert np.array_equal(gc["valid_mask"], small["valid_mask"].reshape(-1).astype(np.float32))
