"""Reference ray caster for the renderer's tests: numpy, written from the definitions in
include/avr.h (the section on avr_render_device), not from the kernel.

It takes the compiled scene's arrays (shape_kind / shape_body / shape_gender / shape_hull /
hull_verts), the shape_pose / shape_param rows of the env's proportions slot, the env's gender, the
body poses and the camera's numbers, builds the hulls' planes itself (scipy.spatial.ConvexHull), and
returns per pixel the ray parameter t of the nearest entering hit, the hit shape's index and the
world normal there.  dtype=np.float64 is the reference; dtype=np.float32 rounds every input to
float32 and keeps all arithmetic in float32: the difference of the two is what fp32 itself costs on
these inputs, the scale of the tests' tolerance (the project's 8x rule).

Imports nothing from avr/render.py: a camera is any object with eye, target, up, fov_y_deg, near,
far, width, height, body.
"""
import numpy as np

SPHERE, CAPSULE, BOX, HULL = 0, 1, 2, 3
BACKGROUND = (204, 230, 255)
# palette by body kind (include/avr.h): robot 0, free 1, static 2, human 3, robot-fixed 4
PALETTE = {0: (190, 195, 205), 1: (240, 200, 60), 2: (140, 150, 160), 3: (230, 170, 140), 4: (190, 195, 205)}


def _rot(q, v):
    """v rotated by the unit quaternion q = (x, y, z, w); v is [..., 3]."""
    u, w = q[:3], q[3]
    t = 2 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def _conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], q.dtype)


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], a.dtype)


def _unit(v):
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def hull_planes(verts):
    """Face planes (n, w), n . x <= w, of the convex hull of verts [nv, 3] (float64, unit n)."""
    from scipy.spatial import ConvexHull
    eq = ConvexHull(np.asarray(verts, np.float64)).equations
    return np.concatenate([eq[:, :3], -eq[:, 3:4]], axis=1)


def camera_frame(cam, body_pose=None, dtype=np.float64):
    """(eye, right, up, forward) in the world.  body_pose: the camera body's [7] frame when cam.body >= 0."""
    eye, tgt, up = (np.asarray(x, dtype) for x in (cam.eye, cam.target, cam.up))
    if cam.body >= 0:
        bp = np.asarray(body_pose, dtype)
        eye, tgt, up = bp[:3] + _rot(bp[3:], eye), bp[:3] + _rot(bp[3:], tgt), _rot(bp[3:], up)
    f = _unit(tgt - eye)
    r = _unit(np.cross(f, up))
    return eye, r, np.cross(r, f), f


def rays(cam, body_pose=None, dtype=np.float64, sub=(0.0, 0.0)):
    """(eye [3], d [H, W, 3] unit) through the pixel centres displaced by sub = (dc, dr) pixels."""
    eye, r, u, f = camera_frame(cam, body_pose, dtype)
    W, H = int(cam.width), int(cam.height)
    k = dtype(np.tan(0.5 * np.deg2rad(np.float64(cam.fov_y_deg))) / H)
    x = ((2 * (np.arange(W) + sub[0]) + 1 - W).astype(dtype) * k)[None, :, None]
    y = ((H - 2 * (np.arange(H) + sub[1]) - 1).astype(dtype) * k)[:, None, None]
    return eye, _unit(f + x * r + y * u)


def _sphere(o, d, r):
    """Entering parameter of |o + t d| = r through the point of closest approach; inf where the ray misses."""
    a = np.sum(d * d, -1)
    tc = -np.sum(o * d, -1) / a
    m = o + tc[:, None] * d
    disc = r * r - np.sum(m * m, -1)
    with np.errstate(invalid='ignore'):
        return np.where(disc >= 0, tc - np.sqrt(np.maximum(disc, 0) / a), np.inf).astype(d.dtype)


def _enter(kind, o, d, par, planes):
    """(t [N], n [N, 3]) of the entering hit of one shape in its own frame; t = inf for a miss."""
    N, dt = len(d), d.dtype
    inf = np.full(N, np.inf, dt)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        if kind == SPHERE:
            t = _sphere(o, d, par[0])
            return t, (o + np.where(np.isfinite(t), t, 0)[:, None] * d) / par[0]
        if kind == CAPSULE:
            r, hh = par[0], par[1]
            t, n = inf.copy(), np.zeros((N, 3), dt)
            # the cylinder |(x, y)| = r between z = -hh and hh
            a = d[:, 0] ** 2 + d[:, 1] ** 2
            ok = a > 1e-12
            a1 = np.where(ok, a, 1)
            tc = -(o[0] * d[:, 0] + o[1] * d[:, 1]) / a1
            mx, my = o[0] + tc * d[:, 0], o[1] + tc * d[:, 1]
            disc = r * r - (mx * mx + my * my)
            tcyl = tc - np.sqrt(np.maximum(disc, 0) / a1)
            z = o[2] + tcyl * d[:, 2]
            hit = ok & (disc >= 0) & (np.abs(z) <= hh)
            t = np.where(hit, tcyl, t)
            n = np.where(hit[:, None], np.stack([(o[0] + tcyl * d[:, 0]) / r, (o[1] + tcyl * d[:, 1]) / r, np.zeros(N, dt)], -1), n)
            # the two caps: the outer half of the spheres at z = +-hh
            for sgn in (1, -1):
                oc = o - np.array([0, 0, sgn * hh], dt)
                ts = _sphere(oc, d, r)
                tz = np.where(np.isfinite(ts), ts, 0)
                z = oc[2] + tz * d[:, 2]
                hit = np.isfinite(ts) & (ts < t) & (sgn * z >= 0)
                t = np.where(hit, ts, t)
                n = np.where(hit[:, None], (oc + tz[:, None] * d) / r, n)
            return t.astype(dt), n.astype(dt)
        if kind == BOX:
            he = par[:3]
            par_ax = d == 0                                        # rays parallel to a slab
            dd = np.where(par_ax, 1, d)
            t1, t2 = (-he - o) / dd, (he - o) / dd
            lo = np.where(par_ax, -np.inf, np.minimum(t1, t2))
            hi = np.where(par_ax, np.where(np.abs(o) > he, -np.inf, np.inf), np.maximum(t1, t2))
            ax = np.argmax(lo, -1)
            tmin, tmax = lo[np.arange(N), ax], hi.min(-1)
            n = np.zeros((N, 3), dt)
            n[np.arange(N), ax] = -np.sign(d[np.arange(N), ax])
            return np.where(tmin <= tmax, tmin, np.inf).astype(dt), n
        # hull: the interval of the ray inside every half space n . x <= w
        P = planes.astype(dt)
        den = d @ P[:, :3].T                                       # [N, np]
        dist = P[:, 3] - P[:, :3] @ o                              # [np]
        tt = dist / np.where(den == 0, 1, den)
        lo = np.where(den < 0, tt, -np.inf)
        hi = np.where(den > 0, tt, np.where((den == 0) & (dist < 0), -np.inf, np.inf))
        ax = np.argmax(lo, -1)
        tmin, tmax = lo[np.arange(N), ax], hi.min(-1)
        return np.where(tmin <= tmax, tmin, np.inf).astype(dt), P[ax, :3]


class Scene:
    """The arrays a render reads, with the hulls' planes built once (float64)."""

    def __init__(self, A, shape_pose=None, shape_param=None):
        self.kind = np.asarray(A['shape_kind'], np.int64)
        self.body = np.asarray(A['shape_body'], np.int64)
        self.gender = np.asarray(A['shape_gender'], np.int64)
        self.body_kind = np.asarray(A['body_kind'], np.int64)
        self.pose = np.asarray(A['shape_pose'] if shape_pose is None else shape_pose, np.float64).reshape(len(self.kind), 7)
        self.param = np.asarray(A['shape_param'] if shape_param is None else shape_param, np.float64).reshape(len(self.kind), 4)
        sh = np.asarray(A['shape_hull'], np.int64).reshape(len(self.kind), 4)
        hv = np.asarray(A['hull_verts'], np.float64).reshape(-1, 3)
        self.planes = {int(s): hull_planes(hv[sh[s, 0]:sh[s, 0] + sh[s, 1]]) for s in np.nonzero(self.kind == HULL)[0]}
        self.hull_radius = {int(s): float(np.sqrt((hv[sh[s, 0]:sh[s, 0] + sh[s, 1]] ** 2).sum(1).max())) for s in self.planes}
        self._bound()

    def _bound(self):
        """Radius of a sphere about each shape frame's origin that holds the shape."""
        k, p = self.kind, self.param
        self.bound = np.where(k == SPHERE, p[:, 0], np.where(k == CAPSULE, p[:, 0] + p[:, 1], np.sqrt((p[:, :3] ** 2).sum(1))))
        for s, r in self.hull_radius.items():
            self.bound[s] = r

    def with_rows(self, shape_pose, shape_param):
        """The same scene with another proportions slot's shape_pose / shape_param rows."""
        S = object.__new__(Scene)
        S.__dict__.update(self.__dict__)
        S.pose = np.asarray(shape_pose, np.float64).reshape(len(self.kind), 7)
        S.param = np.asarray(shape_param, np.float64).reshape(len(self.kind), 4)
        S._bound()
        return S


def trace(scene, gender, poses, cam, dtype=np.float64, sub=(0.0, 0.0)):
    """(t [H, W], id [H, W] int32, n [H, W, 3], d [H, W, 3]): the nearest entering hit with t in
    [near, far] of every pixel's ray over the shapes of `gender` (and the ungendered ones) at the body
    poses [n_bodies, 7]; a miss is t = inf, id = -1; of two shapes at an equal t the lower index wins."""
    dtype = np.dtype(dtype).type
    poses = np.asarray(poses, np.float32).astype(dtype)
    eye, D = rays(cam, poses[cam.body] if cam.body >= 0 else None, dtype, sub)
    H, W = D.shape[:2]
    d = D.reshape(-1, 3)
    d64 = d.astype(np.float64)
    best = np.full(H * W, np.inf, dtype)
    bid = np.full(H * W, -1, np.int32)
    bn = np.zeros((H * W, 3), dtype)
    near, far = dtype(cam.near), dtype(cam.far)
    for s in range(len(scene.kind)):
        if scene.gender[s] >= 0 and scene.gender[s] != gender:
            continue
        bp = poses[scene.body[s]]
        sp = scene.pose[s].astype(np.float32).astype(dtype)
        par = scene.param[s].astype(np.float32).astype(dtype)
        p = bp[:3] + _rot(bp[3:], sp[:3])
        q = _qmul(bp[3:], sp[3:])
        # only the rays that pass the shape's bounding sphere (about its frame's origin) can hit it: the
        # others are skipped, which changes no result (the sphere is padded far beyond rounding)
        w = (p - eye).astype(np.float64)
        pr = d64 @ w
        sel = np.nonzero((w @ w - pr * pr <= (1.01 * scene.bound[s] + 1e-4) ** 2) & (pr > -scene.bound[s] - 1e-4))[0]
        if not len(sel):
            continue
        qc = _conj(q)
        t, n = _enter(int(scene.kind[s]), _rot(qc, eye - p), _rot(qc, d[sel]), par, scene.planes.get(s))
        take = (t >= near) & (t <= far) & (t < best[sel])
        k = sel[take]
        best[k] = t[take]
        bid[k] = s
        bn[k] = _rot(q, n[take])
    return best.reshape(H, W), bid.reshape(H, W), bn.reshape(H, W, 3), D


def shade(n, d):
    """0.3 + 0.7 max(0, -n . d)."""
    return 0.3 + 0.7 * np.maximum(0, -np.sum(n * d, -1))


def facet_shade_range(scene, poses, cam, bid, D, delta):
    """(smin, smax) [H, W]: the shades the definition allows a pixel whose depth is only known to
    +-delta.  On a box or a hull the hit's normal is that of the face the ray enters last; where a
    second face's entry lies within delta of it (the ray passes an edge between two faces closer
    than the depth tolerance) either face's normal is an answer within that tolerance, and the shade
    may be any of theirs.  Elsewhere, and on spheres and capsules, smin = smax = the shade of the
    hit's own normal is left to the caller (NaN here).  float64; poses, bid and the unit rays D as
    trace() takes and returns them."""
    poses = np.asarray(poses, np.float32).astype(np.float64)
    eye = rays(cam, poses[cam.body] if cam.body >= 0 else None, np.float64)[0]
    d = D.reshape(-1, 3).astype(np.float64)
    ids = bid.reshape(-1)
    smin, smax = np.full(len(ids), np.nan), np.full(len(ids), np.nan)
    for s in np.unique(ids[ids >= 0]):
        if scene.kind[s] not in (BOX, HULL):
            continue
        sel = np.nonzero(ids == s)[0]
        bp = poses[scene.body[s]]
        sp = scene.pose[s].astype(np.float32).astype(np.float64)
        par = scene.param[s].astype(np.float32).astype(np.float64)
        p, q = bp[:3] + _rot(bp[3:], sp[:3]), _qmul(bp[3:], sp[3:])
        o, dl = _rot(_conj(q), eye - p), _rot(_conj(q), d[sel])
        with np.errstate(divide='ignore', invalid='ignore'):
            if scene.kind[s] == BOX:
                he = par[:3]
                dd = np.where(dl == 0, 1, dl)
                lo = np.where(dl == 0, -np.inf, np.minimum((-he - o) / dd, (he - o) / dd))
                facing = np.abs(dl)                                   # -n . d of the face entered along each axis
            else:
                P = scene.planes[int(s)]
                den = dl @ P[:, :3].T
                lo = np.where(den < 0, (P[:, 3] - P[:, :3] @ o) / np.where(den == 0, 1, den), -np.inf)
                facing = -den
        cand = lo >= lo.max(-1, keepdims=True) - delta
        sh = 0.3 + 0.7 * np.maximum(0, facing)
        smin[sel] = np.where(cand, sh, np.inf).min(-1)
        smax[sel] = np.where(cand, sh, -np.inf).max(-1)
    return smin.reshape(bid.shape), smax.reshape(bid.shape)


def rgb_of(scene, bid, shade_v):
    """The image the definition gives for hits bid with shade shade_v: float [H, W, 3] before rounding
    (misses: the background)."""
    out = np.empty(bid.shape + (3,), np.float64)
    out[:] = np.array(BACKGROUND, np.float64)
    hit = bid >= 0
    pal = np.array([PALETTE[int(k)] for k in scene.body_kind[scene.body[bid[hit]]]], np.float64).reshape(-1, 3)
    out[hit] = pal * np.asarray(shade_v, np.float64)[hit][:, None]
    return out


SUBS = ((-0.25, -0.25), (0.25, -0.25), (-0.25, 0.25), (0.25, 0.25))


def edge_pixels(scene, gender, poses, cam):
    """[H, W] bool: the pixels where the float64 reference disagrees with itself across the four
    sub-pixel rays at +-1/4 pixel: another id, or depths further apart than a quarter pixel's footprint
    at that depth, t tan(fov_y / 2) / (2 H)."""
    T, I = [], []
    for sub in SUBS:
        t, i, _, _ = trace(scene, gender, poses, cam, np.float64, sub)
        T.append(t)
        I.append(i)
    T, I = np.stack(T), np.stack(I)
    ids_differ = (I != I[0]).any(0)
    hit = (I >= 0).all(0)
    tm = np.where(hit, T, 0)
    foot = tm.mean(0) * np.tan(0.5 * np.deg2rad(cam.fov_y_deg)) / (2 * cam.height)
    return ids_differ | (hit & (tm.max(0) - tm.min(0) > foot))
