"""CPU tests of the XYZ training-target path: the vertex colours and model files of
pix2pose_amd.xyz_model, get_sympose by its properties, the float64 colour restatement (tests/xyz_ref.py) against a ray-cast
oracle that does not share its derivation, and the patch rules (quantisation table, exclusive last row / column, grey fill,
shape formula) on the restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref as D  # noqa: E402
import xyz_ref as X  # noqa: E402

from pix2pose_amd import xyz_model as M  # noqa: E402
from pix2pose_amd.mesh import read_ply, read_ply_rgb, write_ply_rgb  # noqa: E402


# ---- xyz_colors ------------------------------------------------------------------------------------------------------------

def test_extremes_and_centre_of_a_symmetric_box():
    v, _ = D.box_mesh([-40, -30, -15], [40, 30, 15], 2)           # symmetric: the mean is the centre, 0 is a vertex coordinate
    c, norm = M.xyz_colors(v)
    for k in range(3):
        assert np.all(c[v[:, k] == v[:, k].min(), k] == 0) and np.all(c[v[:, k] == v[:, k].max(), k] == 255)
        assert np.all(c[v[:, k] == 0, k] == 127)                  # 127.5 truncates
    assert [norm[a + "_scale"] for a in "xyz"] == [40.0, 30.0, 15.0] and [norm[a + "_ct"] for a in "xyz"] == [0.0, 0.0, 0.0]
    assert set(norm) == set(M.NORM_KEYS) and all(type(x) is float for x in norm.values())


def test_truncation_not_rounding():
    # x spans [-100, 100] around a zero mean; 56.8 maps to ((0.568 + 1) / 2) * 255 = 199.92: truncated to 199, rounded it were 200
    v = np.array([[-100, 0, 0], [100, 0, 0], [56.8, 0, 0], [-56.8, 0, 0], [0, 1, 1], [0, -1, -1]], np.float64)
    c, _ = M.xyz_colors(v)
    assert c[2, 0] == 199 and c[3, 0] == 55
    # the float32 arithmetic of the definition, element by element
    x = v[:, 0].astype(np.float32)
    ct = np.mean(x)
    ab = np.max(np.abs(x - ct))
    want = [int(np.float32(((xi - ct) / ab + 1) / 2 * 255)) for xi in x]
    assert c[:, 0].tolist() == want


def test_off_centre_mesh_uses_the_vertex_mean():
    rs = np.random.RandomState(0)
    v = rs.uniform(-50, 80, (500, 3)) + [10, -20, 300]
    c, norm = M.xyz_colors(v)
    v32 = v.astype(np.float32)
    for k, a in enumerate("xyz"):
        assert norm[a + "_ct"] == float(np.mean(v32[:, k]))
        assert norm[a + "_scale"] == float(np.max(np.abs(v32[:, k] - np.mean(v32[:, k]))))
        far = np.argmax(np.abs(v32[:, k] - np.mean(v32[:, k])))
        assert c[far, k] in (0, 255) and c[:, k].min() >= 0


def test_models_xyz_round_trip(tmp_path):
    models = tmp_path / "models"
    models.mkdir()
    v, t = D.l_mesh(3)
    write_ply_rgb(str(models / "obj_000005.ply"), v, t, np.zeros((len(v), 3), np.uint8))
    v2, t2 = D.box_mesh([-10, -20, -30], [30, 20, 10], 2)
    write_ply_rgb(str(models / "obj_000012.ply"), v2, t2, np.zeros((len(v2), 3), np.uint8))
    out = tmp_path / "models_xyz"
    param = M.write_models_xyz(str(models), str(out))
    assert sorted(param) == [5, 12] and sorted(os.listdir(out)) == ["norm_factor.json", "obj_000005.ply", "obj_000012.ply"]
    assert M.read_norm_factor(str(out / "norm_factor.json")) == param
    for oid, (vv, tt) in ((5, (v, t)), (12, (v2, t2))):
        rv, rt, rc = M.read_xyz_model(str(out / ("obj_%06d.ply" % oid)))
        want, norm = M.xyz_colors(vv)
        assert np.array_equal(rc, want) and rc.dtype == np.uint8 and norm == param[oid]
        assert np.array_equal(rv.astype(np.float32), vv.astype(np.float32)) and np.array_equal(rt, tt)
        pv, pt = read_ply(str(out / ("obj_%06d.ply" % oid)))      # read_ply still returns two values
        assert np.array_equal(pv, rv) and np.array_equal(pt, rt)


def test_ply_reader_colours_ascii_and_absent(tmp_path):
    p = tmp_path / "a.ply"
    p.write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1\n"
                 "property list uchar int vertex_indices\nend_header\n0 0 0 1 2 3\n1 0 0 4 5 6\n0 1 0 255 0 9\n3 0 1 2\n")
    v, t, c = read_ply_rgb(str(p))
    assert c.tolist() == [[1, 2, 3], [4, 5, 6], [255, 0, 9]] and t.tolist() == [[0, 1, 2]] and v.shape == (3, 3)
    q = tmp_path / "b.ply"
    q.write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    assert read_ply_rgb(str(q))[2] is None
    with pytest.raises(ValueError):
        M.read_xyz_model(str(q))


# ---- get_sympose -----------------------------------------------------------------------------------------------------------

def _rotations(n, seed):
    rs = np.random.RandomState(seed)
    return [D.rot(0, rs.uniform(-180, 180)) @ D.rot(1, rs.uniform(-180, 180)) @ D.rot(2, rs.uniform(-180, 180)) for _ in range(n)]


@pytest.mark.parametrize("order", ["xyz", "yxz", "zxy", "xzy", "yzx", "zyx"])
def test_static_euler_round_trip(order):
    for R in _rotations(20, 3):
        a = M.mat2euler_static(R, order)
        assert np.abs(M.euler2mat_static(*a, order) - R).max() < 1e-12
    # static order: the first axis is applied first (rightmost factor)
    i, j, k = ("xyz".index(c) for c in order)
    want = D.rot(k, 30) @ D.rot(j, 20) @ D.rot(i, 10)
    assert np.abs(M.euler2mat_static(np.deg2rad(10), np.deg2rad(20), np.deg2rad(30), order) - want).max() < 1e-15
    # gimbal lock: second angle +-90 degrees still recomposes
    for s in (1, -1):
        R = D.rot(k, 25) @ D.rot(j, 90 * s) @ D.rot(i, -40)
        assert np.abs(M.euler2mat_static(*M.mat2euler_static(R, order), order) - R).max() < 1e-7


def test_sympose_without_symmetry_is_the_identity():
    for R in _rotations(5, 1):
        Rn, lock = M.get_sympose(R, [0, 0, 0, 0, 0, 0])
        assert np.array_equal(Rn, R) and lock is False
        Rn, lock = M.get_sympose(R, [0, 0, -1, 0, 0, 0])          # sum(sym) <= 0: the reference leaves the pose alone
        assert np.array_equal(Rn, R) and lock is False


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_sympose_properties(axis):
    sym = [0.0] * 6
    sym[axis] = 1
    a = np.array(sym[:3])
    locks = 0
    for R in _rotations(40, 10 + axis):
        Rn, lock = M.get_sympose(R, sym)
        assert np.abs(Rn @ Rn.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rn) - 1) < 1e-12       # a rotation
        Q = Rn.T @ R                                                                                       # R = Rn Q
        assert np.abs(Q @ a - a).max() < 1e-12                                                            # Q turns about the axis
        # poses that differ by a turn about the symmetry axis give the same result
        R2, lock2 = M.get_sympose(R @ D.rot(axis, 77.0), sym)
        assert np.abs(R2 - Rn).max() < 1e-12 and lock2 == lock
        assert lock == (abs((Rn @ a)[2]) > 0.8) and abs((Rn @ a)[2] - (R @ a)[2]) < 1e-12
        locks += lock
    assert 0 < locks < 40
    with pytest.raises(ValueError):
        M.get_sympose(np.eye(3), [0, 0, 0.5, 0, 0, 0])


# ---- the colour restatement against the ray-cast oracle --------------------------------------------------------------------

def _xyz_box():
    v, t = D.box_mesh([-40, -30, -15], [40, 30, 15], 3)
    c, norm = M.xyz_colors(v)
    return v, t, c, norm


# (K, H, W, scale of K to that size, nearest and farthest pose in metres)
CASES = [(D.K_640, 120, 160, 4.0, 0.3, 0.6), (D.CAMERAS[3][0], 37, 53, 1.0, 0.1, 0.2)]


def _scaled(K, s):
    K = np.array(K, np.float64)
    K[:2] /= s
    return K


@pytest.mark.parametrize("case", range(len(CASES)))
def test_restated_colour_equals_the_raycast_oracle(case):
    K, H, W, s, zlo, zhi = CASES[case]
    K = _scaled(K, s)
    v, t, c, norm = _xyz_box()
    rs = np.random.RandomState(5 + case)
    n_cmp = 0
    for _ in range(4):
        R, tt = D.random_pose(rs, K, H, W, zlo, zhi)
        color, depth, owner, margin = X.render_xyz(v, t, c, K, R, tt, H, W)
        assert np.array_equal(depth, D.render_depth(v, t, K, R, tt, H, W))            # the depth path's z-buffer, bit for bit
        assert np.array_equal(owner >= 0, depth > 0) and np.all(color[owner < 0] == 0)
        ray, hit = X.raycast_color(v, t, c, K, R, tt, owner)
        # away from edges by depth_ref's margins: the restatement's 1e-4 px and the ray caster's 1e-6 px
        dray, m2 = D.raycast_depth(v, t, K, R, tt, H, W)
        ok = (owner >= 0) & ~margin & ~m2 & (dray > 0)
        n_cmp += int(ok.sum())
        # the restatement's own error: it is compared before the float32 store as well as after it
        assert np.abs(color.astype(np.float64) - ray)[ok].max() <= 2.0 ** -24 + 1e-9
        c64 = _render64(v, t, c, K, R, tt, H, W, owner)
        assert np.abs(c64 - ray)[ok].max() <= 1e-9
    assert n_cmp > 1000


def _render64(v, t, c, K, R, tt, H, W, owner):
    """render_xyz's colour expression for the owning triangle, kept in float64 (no float32 store)."""
    u, vv, zc = D.project(v, K, R, tt)
    col = X.vertex_colors(c).astype(np.float64)
    out = np.zeros((H, W, 3))
    for j, i in zip(*np.nonzero(owner >= 0)):
        f = np.asarray(t)[owner[j, i]][[0, 2, 1]]
        uu, v2, zz, cc = u[f], vv[f], zc[f], col[f]
        A = (uu[1] - uu[0]) * (v2[2] - v2[0]) - (uu[2] - uu[0]) * (v2[1] - v2[0])
        pu, pv = i + 0.5, j + 0.5
        b = [((uu[bb] - uu[a]) * (pv - v2[a]) - (v2[bb] - v2[a]) * (pu - uu[a])) / A for a, bb in ((1, 2), (2, 0), (0, 1))]
        iz = b[0] / zz[0] + b[1] / zz[1] + b[2] / zz[2]
        out[j, i] = [((b[0] * cc[0, k]) / zz[0] + (b[1] * cc[1, k]) / zz[1] + (b[2] * cc[2, k]) / zz[2]) / iz for k in range(3)]
    return out


def test_colour_is_the_normalised_object_coordinate():
    """The property the whole method rests on.  A symmetric box with corner vertices only has the colours 0 and 255, which
    the 8-bit store keeps exactly, so the rendered colour must be ((X / scale) + 1) / 2 of the back-projected surface point X
    (object frame, the renderer's float32 metres) to the bound of the oracle comparison."""
    v, t = D.box_mesh([-40, -30, -15], [40, 30, 15], 1)
    c, norm = M.xyz_colors(v)
    assert set(np.unique(c)) == {0, 255}
    half = D.mesh_metres(v).astype(np.float64).max(axis=0)
    rs = np.random.RandomState(11)
    n = 0
    for K, H, W, s, zlo, zhi in CASES:
        K = _scaled(K, s)
        for _ in range(3):
            R, tt = D.random_pose(rs, K, H, W, zlo, zhi)
            color, depth, owner, margin = X.render_xyz(v, t, c, K, R, tt, H, W)
            _, hit = X.raycast_color(v, t, c, K, R, tt, owner)
            pose = D.gl_pose(tt, R)
            obj = (hit - pose[:3, 3]) @ pose[:3, :3]
            ok = (owner >= 0) & ~margin
            n += int(ok.sum())
            c64 = _render64(v, t, c, K, R, tt, H, W, owner)
            assert np.abs(c64 - (obj / half + 1) / 2)[ok].max() <= 1e-9
            assert np.abs(color - (obj / half + 1) / 2)[ok].max() <= 2.0 ** -24 + 1e-9
    assert n > 1500


def test_colour_on_a_fine_mesh_is_the_coordinate_up_to_the_8_bit_truncation():
    """With vertex colours taken before their 8-bit truncation the property is exact: colour = ((X - ct) / scale + 1) / 2 of the
    back-projected surface point.  The stored uint8 colours add at most 1 / 255 of truncation; checked on the same render."""
    v, t = D.box_mesh([-40, -30, -15], [40, 30, 15], 6)
    c, norm = M.xyz_colors(v)
    K, H, W = _scaled(D.K_640, 4.0), 120, 160
    R, tt = D.random_pose(np.random.RandomState(2), K, H, W, 0.3, 0.5)
    color, depth, owner, margin = X.render_xyz(v, t, c, K, R, tt, H, W)
    _, hit = X.raycast_color(v, t, c, K, R, tt, owner)
    pose = D.gl_pose(tt, R)
    obj_mm = ((hit - pose[:3, 3]) @ pose[:3, :3]) * 1000.0
    ok = (owner >= 0) & ~margin
    assert ok.sum() > 500
    for k, a in enumerate("xyz"):
        want = ((obj_mm[..., k] - norm[a + "_ct"]) / norm[a + "_scale"] + 1) / 2
        err = (want - color[..., k])[ok]
        assert err.min() >= -1e-6 and err.max() <= 1 / 255 + 1e-6          # truncation only lowers a level, by less than one


def test_equal_depth_keeps_the_lower_triangle_index():
    v, t, c = _coplanar_pair()
    K, H, W = D.GRID_K, 480, 640
    color, depth, owner, _ = X.render_xyz(v, t, c, K, np.eye(3), [0, 0, 1000], H, W)
    both = _covered_by(v, t[0:1], K, H, W) & _covered_by(v, t[1:2], K, H, W)
    assert both.sum() > 100 and np.all(owner[both] == 0) and np.all(color[both] == X.vertex_colors(c)[0])
    color2, _, owner2, _ = X.render_xyz(v, t[::-1], c, K, np.eye(3), [0, 0, 1000], H, W)
    assert np.all(owner2[both] == 0) and np.all(color2[both] == X.vertex_colors(c)[3])


def _coplanar_pair():
    """Two overlapping triangles in the plane z = 0 facing a camera on -z, each of one colour."""
    v = np.array([[-250, -250, 0], [250, -250, 0], [0, 250, 0], [-250, 250, 0], [250, 250, 0], [0, -250, 0]], np.float64)
    t = np.array([[0, 2, 1], [3, 4, 5]])
    c = np.array([[255, 0, 0]] * 3 + [[0, 0, 255]] * 3, np.uint8)
    return v, t, c


def _covered_by(v, tris, K, H, W):
    return D.render_depth(v, tris, K, np.eye(3), [0, 0, 1000], H, W) > 0


# ---- patch rules -----------------------------------------------------------------------------------------------------------

def test_quantisation_table_from_its_definition():
    tab = X.quant_table()
    for q in range(256):
        back = np.float32(q) / np.float32(255)            # the float32 read-back of level q
        assert tab[q] == int(np.float32(back * np.float32(255)))       # truncation of the float32 product
        assert tab[q] in (q, q - 1)
    assert tab[0] == 0 and tab[255] == 255
    # a colour goes to its nearest level first
    assert X.quantise(np.float32(0.5)) == tab[128] and X.quantise(np.float32(127.4 / 255)) == tab[127]


def test_patch_crop_fill_and_exclusive_max():
    H, W = 40, 50
    depth = np.zeros((H, W), np.float32)
    depth[10:21, 5:31] = 0.5                              # rows 10..20, columns 5..30
    depth[12, 7] = 0                                      # a hole inside the box
    color = np.zeros((H, W, 3), np.float32)
    color[depth > 0] = [0.25, 0.5, 1.0]
    rgb = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
    bbox = X.bbox_of(depth)
    assert bbox.tolist() == [10, 5, 20, 30]
    p = X.patch_unresized(rgb, color, depth, bbox)
    assert p.shape == (10, 25, 6) and p.dtype == np.uint8          # the last covered row and column are left out
    assert np.array_equal(p[2, 2, :3], [128, 128, 128]) and np.array_equal(p[2, 2, 3:], [0, 0, 0])
    keep = depth[10:20, 5:30] > 0
    assert np.array_equal(p[..., :3][keep], rgb[10:20, 5:30][keep])
    assert np.all(p[..., 3:][keep] == X.quantise(np.float32([0.25, 0.5, 1.0])))
    assert X.bbox_of(np.zeros((H, W))).tolist() == [-1, -1, -1, -1]
    assert X.patch_unresized(rgb, color, np.zeros((H, W), np.float32), [-1, -1, -1, -1]) is None
    one_row = np.zeros((H, W), np.float32)
    one_row[7, 3:9] = 1.0
    assert X.patch_unresized(rgb, color, one_row, X.bbox_of(one_row)) is None      # a zero side


@pytest.mark.parametrize("m,want", [(128, 128), (129, 128), (200, 128), (257, 128)])
def test_patch_shape_formula(m, want):
    assert X.patch_shape(m, m)[0] == want and X.patch_shape(m, 1) == (want, 1 if m <= 128 else int(128.0 / m + 0.5))
    h = m // 2 + 3
    scale = 128.0 / m
    assert X.patch_shape(h, m) == ((h, m) if m <= 128 else (int(h * scale + 0.5), 128))
    assert X.patch_shape(m, h) == ((m, h) if m <= 128 else (128, int(h * scale + 0.5)))


def test_flat_mesh_is_refused():
    with pytest.raises(ValueError, match="flat along z"):
        M.xyz_colors(np.array([[0, 0, 5], [10, 0, 5], [0, 10, 5]], np.float64))
