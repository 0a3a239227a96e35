"""The renderer's host side, without a GPU: the reference ray caster (tests/render_reference.py) against
analytic known answers, the camera helpers and write_png of avr/render.py, and the conditions the GPU
image test (tests/test_gpu_render.py) puts on its own inputs, computed by the reference alone."""
import os
import zlib

import numpy as np
import pytest

from avr import _abi as ABI
from avr import render as RD

import render_reference as RR
import render_util as U


class Cam:
    """A bare camera: the reference needs only the numbers."""

    def __init__(self, eye, target, up=(0, 0, 1), fov_y_deg=60.0, near=0.01, far=10.0, width=9, height=7, body=-1):
        self.eye, self.target, self.up = eye, target, up
        self.fov_y_deg, self.near, self.far, self.width, self.height, self.body = fov_y_deg, near, far, width, height, body


IDENT = (0.0, 0.0, 0.0, 1.0)


def one_shape(kind, param, pose=(0, 0, 0) + IDENT, verts=None, n_bodies=1, body=0):
    """A scene of one shape on body `body`."""
    A = dict(shape_kind=[kind], shape_body=[body], shape_gender=[-1], body_kind=[ABI.BODY_STATIC] * n_bodies, shape_pose=[pose],
             shape_param=[tuple(param) + (0,) * (4 - len(param))], shape_hull=[[0, 0 if verts is None else len(verts), 0, 0]],
             hull_verts=np.zeros((0, 3)) if verts is None else verts)
    return RR.Scene(A)


def centre(img):
    return img[img.shape[0] // 2, img.shape[1] // 2]


# (the reference rounds poses and parameters to float32 first: the known answers hold to about 1e-8)
BODY0 = np.array([[0, 0, 0, 0, 0, 0, 1.0]])


def test_sphere_on_the_axis():
    sc = one_shape(RR.SPHERE, (0.25,))
    cam = Cam((0, -2, 0), (0, 0, 0))
    t, i, n, d = RR.trace(sc, 0, BODY0, cam)
    assert centre(i) == 0 and abs(centre(t) - 1.75) < 1e-7
    assert np.allclose(centre(n), (0, -1, 0), atol=1e-7) and np.allclose(centre(d), (0, 1, 0), atol=1e-7)
    assert abs(RR.shade(centre(n), centre(d)) - 1.0) < 1e-7
    # a ray that passes the centre at distance b hits at sqrt(4 - ...) - sqrt(r^2 - b^2): every pixel against the closed form
    eye = np.array(cam.eye, float)
    b2 = np.sum(np.cross(d, -eye) ** 2, -1)
    want = np.where(b2 <= 0.25 ** 2, np.sum(-eye * d, -1) - np.sqrt(np.maximum(0.25 ** 2 - b2, 0)), np.inf)
    assert np.allclose(t, want, atol=1e-7) and np.array_equal(i >= 0, np.isfinite(want))
    # the eye inside the sphere, or the sphere nearer than `near`: not seen
    assert (RR.trace(sc, 0, BODY0, Cam((0, -0.1, 0), (0, 1, 0)))[1] == -1).all()
    assert centre(RR.trace(sc, 0, BODY0, Cam((0, -2, 0), (0, 0, 0), near=1.8))[1]) == -1
    assert centre(RR.trace(sc, 0, BODY0, Cam((0, -2, 0), (0, 0, 0), far=1.7))[1]) == -1


def test_capsule_side_and_cap():
    sc = one_shape(RR.CAPSULE, (0.1, 0.3))
    t, i, n, _ = RR.trace(sc, 0, BODY0, Cam((0, -2, 0.2), (0, 0, 0.2)))          # the cylinder
    assert centre(i) == 0 and abs(centre(t) - 1.9) < 1e-7 and np.allclose(centre(n), (0, -1, 0), atol=1e-7)
    t, i, n, _ = RR.trace(sc, 0, BODY0, Cam((0, 0, 2), (0, 0, 0), up=(0, 1, 0)))   # the top cap, along the axis
    assert centre(i) == 0 and abs(centre(t) - 1.6) < 1e-7 and np.allclose(centre(n), (0, 0, 1), atol=1e-7)
    t, i, n, _ = RR.trace(sc, 0, BODY0, Cam((0, -2, 0.35), (0, 0, 0.35)))        # the cap from the side: sphere at z = 0.3
    assert abs(centre(t) - (2 - np.sqrt(0.1 ** 2 - 0.05 ** 2))) < 1e-7
    assert np.allclose(centre(n), (0, -np.sqrt(0.75), 0.5), atol=1e-7)
    assert centre(RR.trace(sc, 0, BODY0, Cam((0, -2, 0.41), (0, 0, 0.41)))[1]) == -1   # above the cap


def test_rotated_box_and_hull_of_its_corners():
    he = np.array([0.3, 0.2, 0.1])
    q = (0, 0, np.sin(np.pi / 8), np.cos(np.pi / 8))                              # 45 degrees about z
    box = one_shape(RR.BOX, he, (0.1, 0, 0) + q)
    cam = Cam((0.1, -2, 0.03), (0.1, 0, 0.03), width=31, height=21, fov_y_deg=25)
    t, i, n, d = RR.trace(box, 0, BODY0, cam)
    # the centre ray meets the faces x' = +0.3 / y' = -0.2 of the turned box: the nearer, facing one is
    # y' = -0.2 at world distance 2 - 0.2 sqrt(2) (its plane passes (0.1 + 0.2 sin45, -0.2 cos45))
    assert centre(i) == 0 and abs(centre(t) - (2 - 0.2 * np.sqrt(2))) < 1e-7
    assert np.allclose(centre(n), (np.sqrt(0.5), -np.sqrt(0.5), 0), atol=1e-7)
    corners = np.array([[sx * he[0], sy * he[1], sz * he[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    hull = one_shape(RR.HULL, (0,), (0.1, 0, 0) + q, verts=corners)
    th, ih, nh, _ = RR.trace(hull, 0, BODY0, cam)
    assert np.array_equal(ih, i) and (i >= 0).sum() > 50
    hit = i >= 0
    assert np.abs(th[hit] - t[hit]).max() < 1e-7 and np.abs(nh[hit] - n[hit]).max() < 1e-9


def test_centre_ray_hits_target_and_rows_run_downwards():
    sc = one_shape(RR.SPHERE, (0.05,), (0.3, 0.4, 0.5) + IDENT)
    cam = Cam((1.0, -1.5, 1.2), (0.3, 0.4, 0.5), width=33, height=21)
    t, i, _, d = RR.trace(sc, 0, BODY0, cam)
    dist = np.linalg.norm(np.array(cam.target) - np.array(cam.eye))
    assert centre(i) == 0 and abs(centre(t) - (dist - 0.05)) < 1e-7
    assert d[0, 16, 2] > d[20, 16, 2]                                             # row 0 is the top (up = +z)
    e, r, u, f = RR.camera_frame(cam)
    assert d[10, 32] @ r > 0 > d[10, 0] @ r                                       # columns run to the right
    # square pixels: neighbouring pixel centres are tan(fov / 2) * 2 / H apart on the image plane in both directions
    k = np.tan(np.deg2rad(30.0)) / 21
    p = d / (d @ f)[..., None]
    assert np.allclose((p[10, 17] - p[10, 16]) @ r, 2 * k, atol=1e-7) and np.allclose((p[9, 16] - p[10, 16]) @ u, 2 * k, atol=1e-7)


def test_body_camera_is_the_world_camera_moved_by_the_body():
    rng = np.random.default_rng(3)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    body = np.concatenate([[0.2, -0.1, 0.9], q])
    poses = np.stack([np.array([0, 0, 0, 0, 0, 0, 1.0]), body]).astype(np.float32).astype(np.float64)
    sc = one_shape(RR.BOX, (0.2, 0.3, 0.1), (0.1, 0.5, 0.2) + IDENT, n_bodies=2)
    eye, tgt, up = np.array([0.0, -0.6, 0.3]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])
    on = Cam(eye, tgt, up, body=1, width=15, height=11)
    bq, bp = poses[1, 3:], poses[1, :3]
    world = Cam(bp + RR._rot(bq, eye), bp + RR._rot(bq, tgt), RR._rot(bq, up), width=15, height=11)
    a, b = RR.trace(sc, 0, poses, on), RR.trace(sc, 0, poses, world)
    assert np.array_equal(a[1], b[1]) and (a[1] >= 0).any()
    assert np.allclose(a[0][a[1] >= 0], b[0][b[1] >= 0], atol=1e-7) and np.allclose(a[3], b[3], atol=1e-7)


def test_equal_t_goes_to_the_lower_index():
    A = dict(shape_kind=[RR.SPHERE, RR.BOX, RR.SPHERE], shape_body=[0, 0, 0], shape_gender=[1, -1, -1], body_kind=[ABI.BODY_STATIC],
             shape_pose=[(0, 0, 0) + IDENT] * 3, shape_param=[(0.5, 0, 0, 0), (0.25, 0.25, 0.25, 0), (0.25, 0, 0, 0)],
             shape_hull=[[0, 0, 0, 0]] * 3, hull_verts=np.zeros((0, 3)))
    sc = RR.Scene(A)
    cam = Cam((0, -2, 0), (0, 0, 0))
    # box face y = -0.25 and sphere of radius 0.25 meet the centre ray at the same t = 1.75: shape 1 wins
    t, i, _, _ = RR.trace(sc, 0, BODY0, cam)
    assert centre(t) == 1.75 and centre(i) == 1
    # shape 0 belongs to gender 1 only
    assert centre(RR.trace(sc, 1, BODY0, cam)[1]) == 0 and (RR.trace(sc, 0, BODY0, cam)[1] != 0).all()


def test_float32_mode_rounds_like_float32():
    sc = one_shape(RR.SPHERE, (0.1,), (0.3, 0.1, 0.7) + IDENT)
    cam = Cam((1.0, -1.5, 1.2), (0.3, 0.1, 0.7), width=41, height=31, fov_y_deg=12)
    t64, i64, _, _ = RR.trace(sc, 0, BODY0, cam)
    t32, i32, n32, d32 = RR.trace(sc, 0, BODY0, cam, np.float32)
    assert t32.dtype == np.float32 and n32.dtype == np.float32 and d32.dtype == np.float32
    hit = (i64 >= 0) & (i32 >= 0)
    err = np.abs(t32[hit].astype(np.float64) - t64[hit])
    assert hit.sum() > 100 and 0 < err.max() < 1e-4


def test_from_yaw_pitch_and_default_cameras():
    c = RD.Camera.from_yaw_pitch(2.0, 0.0, 0.0, (0.1, 0.2, 0.3))
    assert np.allclose(c.eye, (0.1, -1.8, 0.3)) and np.allclose(c.target, (0.1, 0.2, 0.3)) and c.up == (0.0, 0.0, 1.0) and c.body == -1
    assert np.allclose(RR.camera_frame(c)[3], (0, 1, 0))                           # yaw 0, pitch 0 looks along +y
    c = RD.Camera.from_yaw_pitch(1.0, 90.0, -30.0, (0, 0, 0))
    assert np.allclose(RR.camera_frame(c)[3], (-np.cos(np.pi / 6), 0, -0.5), atol=1e-7)
    f = RD.default_camera(ABI.TASK_FEEDING)
    assert f == RD.default_camera(ABI.TASK_BEDBATH) and np.allclose(f.target, (-0.2, 0, 0.75))
    assert abs(np.linalg.norm(np.subtract(f.eye, f.target)) - 1.10) < 1e-7 and (f.fov_y_deg, f.near, f.far) == (60.0, 0.01, 10.0)
    s = RD.default_camera(ABI.TASK_SCRATCH)
    assert abs(np.linalg.norm(np.subtract(s.eye, s.target)) - 1.75) < 1e-7 and np.allclose(s.target, (-0.2, 0, 0.4))
    with pytest.raises(NotImplementedError):
        RD.default_camera(ABI.TASK_DRESSING)
    b = RD.Camera.on_body(5, (0, 0, 1), (0, 1, 0)).resized(48, 32)
    assert (b.body, b.width, b.height) == (5, 48, 32)


def test_write_png_decodes_back(tmp_path):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    path = os.path.join(tmp_path, 'a.png')
    RD.write_png(path, img)
    b = open(path, 'rb').read()
    assert b[:8] == b'\x89PNG\r\n\x1a\n' and b[12:16] == b'IHDR' and int.from_bytes(b[16:20], 'big') == 17 and int.from_bytes(b[20:24], 'big') == 13
    i = b.index(b'IDAT')
    n = int.from_bytes(b[i - 4:i], 'big')
    raw = np.frombuffer(zlib.decompress(b[i + 4:i + 4 + n]), np.uint8).reshape(13, 1 + 3 * 17)
    assert not raw[:, 0].any() and np.array_equal(raw[:, 1:].reshape(13, 17, 3), img)
    assert int.from_bytes(b[i + 4 + n:i + 8 + n], 'big') == zlib.crc32(b[i:i + 4 + n])
    assert np.array_equal(RD.read_png(path), img)
    sheet = RD.contact_sheet(np.stack([img] * 5), cols=3)
    assert sheet.shape == (2 * 15 + 2, 3 * 19 + 2, 3) and np.array_equal(sheet[2:15, 2:19], img) and tuple(sheet[0, 0]) == RD.BACKGROUND
    with pytest.raises(ValueError):
        RD.write_png(path, img[..., 0])


def test_hull_planes_follow_the_model_compilers_merging_rule():
    from avr import model_compiler as MC
    A, md = U.scene(ABI.TASK_SCRATCH)
    P, R = RD.hull_planes(A)
    kind, sh = np.asarray(A['shape_kind']), np.asarray(A['shape_hull']).reshape(-1, 4)
    assert np.array_equal(R[:, 1] > 0, kind == RD.HULL) and R[kind == RD.HULL, 1].min() >= 4 and R[:, 1].sum() == len(P)
    assert np.allclose(np.linalg.norm(P[:, :3], axis=1), 1.0, atol=1e-7)
    for s in np.nonzero(kind == RD.HULL)[0][::23]:
        v = np.asarray(A['hull_verts'])[sh[s, 0]:sh[s, 0] + sh[s, 1]]
        mine = P[R[s, 0]:R[s, 0] + R[s, 1]]
        assert np.array_equal(mine, MC.Hull(v).planes)
        assert (v @ mine[:, :3].T - mine[:, 3]).max() < 1e-9                     # every vertex inside every plane
    assert RD.hull_planes(A)[0] is P                                               # cached per scene
    T = RD.shape_table(md)
    assert len(T['label']) == len(kind) and set(np.unique(T['kind'])) <= set(RD.PALETTE)
    assert T['label'][int(np.nonzero(T['kind'] == ABI.BODY_ROBOT)[0][0])].startswith('robot link')


def test_variant_scenes_keep_the_base_hulls():
    from avr import model_compiler as MC
    A, _ = U.scene(ABI.TASK_FEEDING)
    R = MC.human_variant_records('feeding_jaco', 'male', 0.50)
    RD.assert_variant_hulls(A, R['arrays'])
    assert not np.array_equal(R['shape_param'], np.asarray(A['shape_param'], np.float32)[R['shapes']])
    bad = dict(R['arrays'], hull_verts=np.asarray(R['arrays']['hull_verts']) * 1.01)
    with pytest.raises(AssertionError):
        RD.assert_variant_hulls(A, bad)


def condition_figures(task, name, poses, gender):
    """(edge share, {kind: non-edge pixels}) of one image by the reference alone."""
    A, _ = U.scene(task)
    sc = scene_of(task)
    cam = U.case_camera(task, name, poses)
    edge = RR.edge_pixels(sc, gender, poses, cam)
    return float(edge.mean()), U.coverage(A, RR.trace(sc, gender, poses, cam)[1], ~edge)


_SCENES = {}


def scene_of(task):
    if task not in _SCENES:
        _SCENES[task] = RR.Scene(U.scene(task)[0])
    return _SCENES[task]


def test_edge_share_and_coverage_conditions_of_the_gpu_cases(oracle_built):
    """The conditions the GPU image test puts on its inputs, for every (task, camera) it uses, at the
    reset states and the host's body poses: at most 25 % edge pixels, and at least 20 non-edge pixels
    on each of robot, human, static and tool / free bodies.

    The depth clause of an edge pixel (four sub-pixel depths further apart than a quarter pixel's
    footprint f = t tan(fov_y / 2) / (2 H)) is met by every smooth surface whose normal makes more than
    about 27 degrees with the ray, at any resolution and field of view: a surface at the angle a spreads
    the depths by about 2 f tan(a).  The tasks' GUI cameras come out at 0.91 - 0.94 edge share and a head
    camera looking forward at 0.44 - 0.82, so the cases use the views of tests/render_util.py, which
    look down on the env's tool (render_util.VIEW, case_camera; the head case 10 degrees off the
    vertical): floor, lap, bed and the links' and tools' tops face them.  Figures at the reset states
    (edge share; non-edge pixels on robot / human / static / tool-free):
      FeedingJaco     132 x 88  world (env 1, a woman) 0.224; 611 / 192 / 8035 / 178   head (env 2, a man) 0.245; 573 / 192 / 7749 / 261
      ScratchItchPR2  160 x 64  world (env 0, a man)   0.209; 406 / 119 /  238 / 161   head (env 1, a woman) 0.171; 441 / 112 / 175 / 161
      BedBathingPR2    96 x 64  world (env 0, a man)   0.208; 499 /  42 / 1369 / 190   head (env 1, a woman) 0.150; 463 /  30 / 872 / 173"""
    bad = []
    for task in U.TASKS:
        _, md = U.scene(task)
        S = U.reset_states(task)
        for name in U.CASES:
            e = U.case_env(task, name)
            poses = U.host_body_poses(task, S[e]).astype(np.float32)
            share, cov = condition_figures(task, name, poses, int(S[e, md.layout.S_TASK + md.layout.T_GENDER]))
            line = '%s %s: edge share %.3f, non-edge pixels %s' % (U.TASK_NAMES[task], name, share, cov)
            print(line)
            if share > U.EDGE_CAP or min(cov.values()) < U.MIN_PIXELS:
                bad.append(line)
    assert not bad, '\n'.join(bad)


def test_facet_shade_range_opens_only_at_a_face_edge():
    """A box turned 45 degrees and looked at along its edge: the centre ray enters two faces at the
    same t: the pixels beside the edge (the faces' entries 0.04 m apart) may take either face's shade
    once the depth tolerance reaches that, the pixels further out only under a tolerance as large as
    the box, and none under a tolerance of a micron."""
    q = (0, 0, np.sin(np.pi / 8), np.cos(np.pi / 8))
    sc = one_shape(RR.BOX, (0.2, 0.2, 0.2), (0, 0, 0) + q)
    cam = Cam((0.0, -2, 0.0), (0.0, 0, 0.0), width=20, height=5, fov_y_deg=6)
    t, i, n, d = RR.trace(sc, 0, BODY0, cam)
    s = RR.shade(n, d)
    hit = i >= 0
    assert hit[2, 5] and hit[2, 9] and hit[2, 10] and hit[2, 14]
    for delta, open_cols, closed_cols in ((1e-6, (), (5, 9, 10, 14)), (0.05, (9, 10), (5, 14)), (1.0, (5, 9, 10, 14), ())):
        lo, hi = RR.facet_shade_range(sc, BODY0, cam, i, d, delta)
        assert np.all(lo[hit] <= s[hit] + 1e-12) and np.all(s[hit] <= hi[hit] + 1e-12)
        assert all((hi - lo)[2, c] > 1e-3 for c in open_cols) and all((hi - lo)[2, c] < 1e-12 for c in closed_cols), delta
    sph = one_shape(RR.SPHERE, (0.25,))
    ts, is_, ns, ds = RR.trace(sph, 0, BODY0, Cam((0, -2, 0), (0, 0, 0)))
    assert np.isnan(RR.facet_shade_range(sph, BODY0, Cam((0, -2, 0), (0, 0, 0)), is_, ds, 1e-3)[0]).all()
