"""CPU tests of the depth path: the PLY reader and self-checks of the float64 restatement (tests/depth_ref.py) that the GPU
tests hold the rasteriser and the depth score to."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref as D  # noqa: E402

from pix2pose_amd.mesh import read_ply  # noqa: E402

# a unit cube's top as one quad plus a triangle, with normals / colours and an extra element the reader must skip
VERTS = np.array([[0, 0, 0], [10, 0, 0], [10, 10, 0], [0, 10, 0], [5, 5, 7.25]], np.float64)
FACES = [[0, 1, 2, 3], [0, 1, 4]]
FAN = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4]])


def _write_ascii(fn):
    lines = ["ply", "format ascii 1.0", "comment made by the test", "element vertex %d" % len(VERTS), "property float x",
             "property float y", "property float z", "property float nx", "property uchar red",
             "element face %d" % len(FACES), "property list uchar int vertex_indices", "property uchar flags",
             "element edge 1", "property int vertex1", "property int vertex2", "end_header"]
    lines += ["%g %g %g 0.5 200" % tuple(v) for v in VERTS]
    lines += ["%d %s 3" % (len(f), " ".join(map(str, f))) for f in FACES]
    lines += ["0 1"]
    open(fn, "w").write("\n".join(lines) + "\n")


def _write_binary(fn, quads_only=False):
    faces = [[0, 1, 2, 3], [1, 2, 3, 4]] if quads_only else FACES
    hdr = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(VERTS), "property float x", "property float y",
           "property float z", "property double nx", "property uchar red", "element face %d" % len(faces),
           "property list uchar int vertex_indices", "end_header"]
    b = ("\n".join(hdr) + "\n").encode()
    for v in VERTS:
        b += struct.pack("<fffdB", v[0], v[1], v[2], 0.25, 7)
    for f in faces:
        b += struct.pack("<B%di" % len(f), len(f), *f)
    open(fn, "wb").write(b)
    return faces


def test_ply_ascii_with_quads_and_extra_properties(tmp_path):
    fn = str(tmp_path / "obj_000001.ply")
    _write_ascii(fn)
    v, t = read_ply(fn)
    assert np.array_equal(v, VERTS.astype(np.float32).astype(np.float64))
    assert np.array_equal(t, FAN) and t.dtype == np.int32


def test_ply_binary_little_endian_mixed_and_quads(tmp_path):
    fn = str(tmp_path / "obj_000002.ply")
    _write_binary(fn)
    v, t = read_ply(fn)
    assert np.array_equal(v, VERTS.astype(np.float32).astype(np.float64))
    assert np.array_equal(t, FAN)
    fn2 = str(tmp_path / "obj_000003.ply")
    _write_binary(fn2, quads_only=True)         # every polygon the same size: the vectorised path
    _, t2 = read_ply(fn2)
    assert np.array_equal(t2, [[0, 1, 2], [0, 2, 3], [1, 2, 3], [1, 3, 4]])


def test_restatement_culls_back_faces_of_an_outward_mesh():
    """A closed box wound outward, 500 mm in front of the camera: the centre pixel sees the near face.  With the winding
    flipped the near face is culled and the inside of the far face is what is drawn."""
    v, t = D.box_mesh([-50, -50, -50], [50, 50, 50], 2)
    K = D.K_640
    d = D.render_depth(v, t, K, np.eye(3), [0, 0, 500], 480, 640)        # t in mm, as p2p_refine_job carries it
    j, i = int(K[1, 2]), int(K[0, 2])
    assert abs(d[j, i] - 0.45) < 1e-6
    dflip = D.render_depth(v, t[:, ::-1], K, np.eye(3), [0, 0, 500], 480, 640)
    assert abs(dflip[j, i] - 0.55) < 1e-6
    assert np.array_equal(d > 0, dflip > 0)      # same silhouette


def test_restatement_depth_of_a_tilted_plane_is_the_ray_intersection():
    """Perspective-correct depth: every covered pixel of a tilted square sits on the plane, and the shared diagonal leaves no hole."""
    verts = np.array([[-60, -60, 0], [60, -60, 0], [60, 60, 0], [-60, 60, 0]], np.float64)
    tris = np.array([[0, 1, 2], [0, 2, 3]])
    R = D.rot(0, 35) @ D.rot(1, -20)
    if (R @ [0, 0, 1])[2] > 0:                   # show the front (+z normal must face the camera)
        tris = tris[:, ::-1]
    t = np.array([0.01, -0.02, 0.4])
    K = D.K_640
    d = D.render_depth(verts, tris, K, R, t * 1000.0, 480, 640)
    n = R @ [0, 0, 1.0]
    vm = D.mesh_metres(verts).astype(np.float64)
    c = vm[0] @ R.T + t
    jj, ii = np.nonzero(d > 0)
    assert len(jj) > 5000
    rays = np.linalg.solve(K, np.stack([ii + 0.5, jj + 0.5, np.ones(len(ii))]))      # OpenGL pixel centres
    z = (c @ n) / (n @ rays)
    assert np.abs(d[jj, ii] - z).max() < 1e-6 * z.max()
    # no hole inside the projected square: pixels whose centre is well inside the quad are all covered
    P = (K @ (vm @ R.T + t).T)
    uv = (P[:2] / P[2]).T
    pu, pv = np.meshgrid(np.arange(640) + 0.5, np.arange(480) + 0.5)
    es = []
    for a in range(4):
        b = (a + 1) % 4
        du, dv = uv[b] - uv[a]
        es.append((du * (pv - uv[a, 1]) - dv * (pu - uv[a, 0])) / np.hypot(du, dv))
    es = np.array(es)
    inside = np.all(es > 1e-3, 0) | np.all(es < -1e-3, 0)
    assert inside.sum() > 5000 and np.all(d[inside] > 0)


def test_restatement_clips_and_rejects_without_failing():
    v, t = D.l_mesh(4)
    K = D.K_640
    # straddling the near plane and far out of the image: nothing raises, depths stay within the clip range
    for tt in ([0, 0, 20], [3000, 0, 300], [0, 0, 12000], [0, 0, -1000]):
        d = D.render_depth(v, t, K, D.rot(1, 10), tt, 480, 640)
        assert np.all((d == 0) | ((d >= 0.01) & (d <= 10)))
    assert not D.render_depth(v, t, K, np.eye(3), [0, 0, 12000], 480, 640).any()        # beyond the far plane
    assert not D.render_depth(v, t, K, np.eye(3), [0, 0, -1000], 480, 640).any()        # behind the camera


def test_unit_quirk_of_render_obj_is_kept():
    """render_obj gets tra_pred/1000 and divides once more when that exceeds 100 (icp3d.py:46): a t_z beyond 100 m is drawn 1000x nearer."""
    v, t = D.l_mesh(2)
    a = D.render_depth(v, t, D.K_640, D.rot(2, 30), [10000.0, -5000.0, 700000.0], 480, 640)
    b = D.render_depth(v, t, D.K_640, D.rot(2, 30), [10.0, -5.0, 700.0], 480, 640)
    both = (a > 0) & (b > 0)
    assert both.sum() > 100 and ((a > 0) != (b > 0)).sum() <= 5          # the two divisions round differently: edge centres may flip
    assert np.abs(a[both] - b[both]).max() <= 1e-6 * b.max()


def test_tie_rule_gives_every_centre_exactly_one_write():
    """Vertices exactly on pixel centres: all edges run through centres.  Counted independently of the depth: every centre of
    the 64 x 64 px square is written by exactly one triangle (no hole on a shared edge, no double write), and of each pair of
    opposite outer edges exactly one owns its centres, so the square covers exactly 64 x 64 pixels."""
    v, t = D.pixel_grid_mesh()
    vm = D.mesh_metres(v)
    assert set(np.unique(vm[:, :2])) == {-0.5, -0.25, 0.0, 0.25, 0.5}            # exact: the vertices sit on centres
    d, counts = D.render_depth(v, t, D.GRID_K, np.eye(3), [0, 0, 1000], 480, 640, with_counts=True)
    assert counts.max() == 1 and counts.sum() == 64 * 64
    jj, ii = np.nonzero(counts)
    assert ii.max() - ii.min() == 63 and jj.max() - jj.min() == 63
    assert np.all(d[counts == 1] == 1.0) and not d[counts == 0].any()


def test_depth_score_restatement_by_hand():
    ref = np.array([[0.5, 0.5, 0.0], [0.5, 0.6, 0.7]], np.float32)
    tgt = np.array([[0.51, 0.5, 0.3], [0.525, 0.6, 0.0]], np.float32)
    m = np.array([[1, 1, 1], [1, 0, 1]], np.uint8)
    s, inl = D.depth_score(ref, tgt, m)
    assert s["union"] == 5 and s["inlier_count"] == 2
    assert np.array_equal(inl, [[True, True, False], [False, False, False]])
    d = np.abs(np.float64(np.float32(0.51)) - np.float64(np.float32(0.5)))
    assert abs(s["fcn"] - ((0.02 - d) / 0.02 + 1.0)) < 1e-12
    assert s["ratio"] == 2 / 5
