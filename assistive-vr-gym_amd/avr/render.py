"""Views of the envs: cameras, the hulls' face planes and the helpers around avr_render_device
(include/avr.h; csrc/avr_render.hip).

The reference shows its world only through Bullet's GUI (env.py:613-620); here a handle ray-casts
its own collision geometry into depth, shape-id and RGB images.  `AVRVecEnv.render` /
`AVRTorchVecEnv.render_device` (avr/env.py) are the public faces; this module holds what they share.
"""
import dataclasses
import hashlib
import struct
import zlib

import numpy as np

from . import _abi as ABI

BACKGROUND = (204, 230, 255)        # the reference GUI's background (env.py:618)
# include/avr.h: palette by the hit body's kind (index: _abi.BODY_*)
PALETTE = {ABI.BODY_ROBOT: (190, 195, 205), ABI.BODY_RSTATIC: (190, 195, 205), ABI.BODY_FREE: (240, 200, 60),
           ABI.BODY_HUMAN: (230, 170, 140), ABI.BODY_STATIC: (140, 150, 160)}
BODY_KIND_NAMES = {ABI.BODY_ROBOT: 'robot', ABI.BODY_FREE: 'free', ABI.BODY_STATIC: 'static', ABI.BODY_HUMAN: 'human', ABI.BODY_RSTATIC: 'robot-fixed'}
HULL = 3                            # include/avr_model.h AVR_HULL
HEAD_LINK = 27                      # the human's head link (human_creation.py; FeedingJaco's task_head_link)


@dataclasses.dataclass
class Camera:
    """include/avr.h avr_camera: a pinhole with square pixels.  body = -1: eye, target, up are world
    coordinates; body >= 0: they are given in that collision body's COM frame of each rendered env."""
    eye: tuple
    target: tuple
    up: tuple = (0.0, 0.0, 1.0)
    fov_y_deg: float = 60.0         # this build's choice: the reference's GUI camera has no stated field of view
    near: float = 0.01
    far: float = 10.0
    width: int = 320
    height: int = 240
    body: int = -1

    @classmethod
    def world(cls, eye, target, up=(0.0, 0.0, 1.0), **kw):
        return cls(tuple(float(x) for x in eye), tuple(float(x) for x in target), tuple(float(x) for x in up), body=-1, **kw)

    @classmethod
    def on_body(cls, body, eye, target, up=(0.0, 0.0, 1.0), **kw):
        """A camera riding on collision body `body`: eye, target, up in that body's COM frame."""
        return cls(tuple(float(x) for x in eye), tuple(float(x) for x in target), tuple(float(x) for x in up), body=int(body), **kw)

    @classmethod
    def from_yaw_pitch(cls, distance, yaw, pitch, target, **kw):
        """p.resetDebugVisualizerCamera's arguments (degrees) for a z-up world: the camera looks along
        f = (-sin yaw cos pitch, cos yaw cos pitch, sin pitch) at `target` from `distance` away, up +z.
        Our reading of Bullet's convention (DESIGN: unpinned against a Bullet screenshot)."""
        y, p = np.deg2rad(float(yaw)), np.deg2rad(float(pitch))
        f = np.array([-np.sin(y) * np.cos(p), np.cos(y) * np.cos(p), np.sin(p)])
        t = np.asarray(target, float)
        return cls.world(t - float(distance) * f, t, (0.0, 0.0, 1.0), **kw)

    def resized(self, width, height):
        return dataclasses.replace(self, width=int(width), height=int(height))


def default_camera(task, **kw):
    """The reference's GUI camera of each task: FeedingJaco and BedBathingPR2 distance 1.10, yaw 40,
    pitch -45 at [-0.2, 0, 0.75] (feeding.py:264, bed_bathing.py:220), ScratchItchPR2 the world
    creation's distance 1.75, yaw -25, pitch -45 at [-0.2, 0, 0.4] (world_creation.py:31)."""
    if task == ABI.TASK_SCRATCH:
        return Camera.from_yaw_pitch(1.75, -25.0, -45.0, (-0.2, 0.0, 0.4), **kw)
    if task in (ABI.TASK_FEEDING, ABI.TASK_BEDBATH):
        return Camera.from_yaw_pitch(1.10, 40.0, -45.0, (-0.2, 0.0, 0.75), **kw)
    raise NotImplementedError('render: not built for task %r' % (task,))


def merged_planes(pts):
    """Face planes [n, 4] = (n, w), n . x <= w, of the convex hull of pts with model_compiler.Hull's
    merging rule: a facet whose plane repeats an earlier kept one (normals within 1e-9 in the dot
    product, offsets within 1e-9) is dropped.  The same planes in the same order as Hull(pts).planes,
    with the comparison against the kept planes vectorised (the largest hull has 2088 of them)."""
    from scipy.spatial import ConvexHull
    eq = ConvexHull(np.asarray(pts, float)).equations
    K, nk = np.zeros((len(eq), 4)), 0
    for e in eq:
        n, d = e[:3], -e[3]
        if nk and np.any((K[:nk, :3] @ n > 1.0 - 1e-9) & (np.abs(K[:nk, 3] - d) < 1e-9)):
            continue
        K[nk, :3], K[nk, 3] = n, d
        nk += 1
    return K[:nk].copy()


_PLANES = {}     # per scene in the process: digest of the hull tables -> (planes4, range2)


def hull_planes(A):
    """(planes4 float64 [n_planes, 4], range2 int32 [n_shapes, 2]) of a compiled scene: for every hull
    shape the face planes n . x <= w of its hull_verts' convex hull in the shape's frame (the core,
    without the collision margin), coplanar facets merged by model_compiler.Hull's rule; range2 rows
    are (first plane, count), count 0 for shapes that are no hull.  Cached per scene."""
    kind = np.asarray(A['shape_kind'])
    sh = np.asarray(A['shape_hull'], np.int64).reshape(len(kind), 4)
    hv = np.ascontiguousarray(A['hull_verts'], np.float64).reshape(-1, 3)
    key = hashlib.sha1(hv.tobytes() + sh.tobytes() + kind.astype(np.int64).tobytes()).hexdigest()
    if key not in _PLANES:
        planes, rng = [], np.zeros((len(kind), 2), np.int32)
        n = 0
        for s in np.nonzero(kind == HULL)[0]:
            P = merged_planes(hv[sh[s, 0]:sh[s, 0] + sh[s, 1]])
            rng[s] = (n, len(P))
            n += len(P)
            planes.append(P)
        _PLANES[key] = (np.concatenate(planes) if planes else np.zeros((0, 4)), rng)
    return _PLANES[key]


def install_planes(sim, A):
    """Install scene A's hull planes in the handle, once (the first render of a handle)."""
    if not getattr(sim, '_render_planes', False):
        P, R = hull_planes(A)
        sim.render_set_planes(P, R)
        sim._render_planes = True


def assert_variant_hulls(base, variant):
    """A height variant's scene has the base scene's hulls: the same hull_verts and per-shape vertex
    ranges, so the base planes serve every variant and only shape_pose / shape_param differ per row."""
    for k in ('shape_kind', 'shape_hull', 'hull_verts'):
        if not np.array_equal(np.asarray(base[k]), np.asarray(variant[k])):
            raise AssertionError('height variant: %s differs from the base scene; its hulls need their own planes' % k)


def shape_table(md):
    """What an id image's values mean: for every shape index its collision body, that body's kind
    (_abi.BODY_*), the body's index within its kind (robot link, free body, static body or human slot)
    and a label; arrays of length n_shapes (index -1, a miss, is not a row)."""
    A = md.A
    body = np.asarray(A['shape_body'], np.int64)
    bk = np.asarray(A['body_kind'], np.int64)[body]
    bi = np.asarray(A['body_index'], np.int64)[body]
    unit = {ABI.BODY_ROBOT: 'link', ABI.BODY_FREE: 'body', ABI.BODY_STATIC: 'body', ABI.BODY_HUMAN: 'slot', ABI.BODY_RSTATIC: 'part'}
    label = ['%s %s %d' % (BODY_KIND_NAMES[int(k)], unit[int(k)], int(i)) for k, i in zip(bk, bi)]
    return dict(body=body, kind=bk, index=bi, label=label)


def head_body(A, md):
    """The collision body of the human's head: the human slot of link 27 (human_creation.py's head,
    FeedingJaco's task_head_link; the PR2 tasks' scenes build the same human and name no head slot)."""
    bk, bi = np.asarray(A['body_kind']), np.asarray(A['body_index'])
    slot = int(md.desc.head_slot)
    if slot < 0:
        slot = int(np.nonzero(np.asarray(A['human_slot_link']) == HEAD_LINK)[0][0])
    hb = np.nonzero(bk == ABI.BODY_HUMAN)[0]
    return int(hb[bi[hb] == slot][0])


def write_png(path, rgb):
    """An [H, W, 3] uint8 array as an 8-bit RGB PNG (zlib only: no imaging library)."""
    a = np.ascontiguousarray(rgb, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('write_png: expected [H, W, 3] uint8, got %r' % (a.shape,))
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, 3 * w)], axis=1).tobytes()   # filter type 0 per row

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)

    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw, 6))
                + chunk(b'IEND', b''))


def read_png(path):
    """The inverse of write_png for its own files (8-bit RGB, filter 0): [H, W, 3] uint8."""
    b = open(path, 'rb').read()
    if b[:8] != b'\x89PNG\r\n\x1a\n':
        raise ValueError('%s: not a PNG' % path)
    p, idat, w, h = 8, b'', 0, 0
    while p < len(b):
        n, tag = struct.unpack('>I', b[p:p + 4])[0], b[p + 4:p + 8]
        data = b[p + 8:p + 8 + n]
        if tag == b'IHDR':
            w, h, depth, ctype = struct.unpack('>IIBB', data[:10])
            if (depth, ctype) != (8, 2):
                raise ValueError('%s: not 8-bit RGB' % path)
        elif tag == b'IDAT':
            idat += data
        p += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    if rows[:, 0].any():
        raise ValueError('%s: filtered rows (not written by write_png)' % path)
    return rows[:, 1:].reshape(h, w, 3).copy()


def contact_sheet(frames, cols=None, pad=2):
    """Frames [N, H, W, 3] tiled into one image, `cols` per row, on the background colour."""
    F = np.asarray(frames, np.uint8)
    n, h, w = F.shape[:3]
    cols = int(cols or min(n, 8))
    rows = -(-n // cols)
    out = np.empty((rows * (h + pad) + pad, cols * (w + pad) + pad, 3), np.uint8)
    out[:] = np.array(BACKGROUND, np.uint8)
    for i in range(n):
        r, c = divmod(i, cols)
        out[pad + r * (h + pad):pad + r * (h + pad) + h, pad + c * (w + pad):pad + c * (w + pad) + w] = F[i]
    return out


def render_host(sim, A, cam, env_ids=None, outputs=('rgb',), device=0):
    """Render through the handle into fresh device buffers and copy them to the host (blocks):
    {name: array} for the names in outputs ('depth' [n, H, W] float32, 'id' [n, H, W] int32, 'rgb'
    [n, H, W, 3] uint8).  torch owns the device buffers."""
    import torch
    bad = [o for o in outputs if o not in ('depth', 'id', 'rgb')]
    if bad or not outputs:
        raise ValueError("render: outputs must name some of 'depth', 'id', 'rgb', not %r" % (tuple(outputs),))
    install_planes(sim, A)
    n = sim.n if env_ids is None else len(env_ids)
    dev = torch.device('cuda', int(device))
    H, W = int(cam.height), int(cam.width)
    buf = {}
    if 'depth' in outputs:
        buf['depth'] = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    if 'id' in outputs:
        buf['id'] = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    if 'rgb' in outputs:
        buf['rgb'] = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    ext = torch.cuda.ExternalStream(sim.stream(), device=dev)
    ext.wait_stream(torch.cuda.current_stream(dev))
    ptr = {k: (buf[k].data_ptr() if k in buf else None) for k in ('depth', 'id', 'rgb')}
    sim.render_device(cam, env_ids, ptr['depth'], ptr['id'], ptr['rgb'], n=n)
    sim.sync()
    return {k: v.cpu().numpy() for k, v in buf.items()}
