"""Shared inputs of the renderer's tests: the reset states, the cameras and the host body poses of
every (task, camera) case, so that the CPU test pins the conditions of exactly the cases the GPU test
runs."""
import functools

import numpy as np

from avr import _abi as ABI
from avr import render as RD

TASKS = (ABI.TASK_FEEDING, ABI.TASK_SCRATCH, ABI.TASK_BEDBATH)
TASK_NAMES = {ABI.TASK_FEEDING: 'FeedingJaco', ABI.TASK_SCRATCH: 'ScratchItchPR2', ABI.TASK_BEDBATH: 'BedBathingPR2'}
N_ENVS = 4
GENDERS = ['male', 'female', 'male', 'female']
# the reset draws' env ids: in the PR2 tasks envs 0 and 1 share the draws of id 0 (the one base pose of
# the four that leaves the tool in sight from above), so that a man and a woman are both rendered
ENV_IDS = {ABI.TASK_FEEDING: [0, 0, 2, 2], ABI.TASK_SCRATCH: [0, 0, 2, 3], ABI.TASK_BEDBATH: [0, 0, 2, 3]}
EDGE_CAP = 0.25          # at most this share of an image's pixels may be edge pixels
MIN_PIXELS = 20          # non-edge pixels compared on each of robot, human, static, tool / free
HULL_MARGIN = 1e-3       # the model's hull margin: the tolerance itself must stay below it


@functools.lru_cache(maxsize=None)
def scene(task):
    A = ABI.load_scene(task)
    return A, ABI.ModelDesc(A)


@functools.lru_cache(maxsize=None)
def reset_states(task):
    """N_ENVS reset states of the task (float32 rows), men and women in turn, envs 2 and 3 of FeedingJaco
    with the tremor-driven head chain; host code only."""
    A, md = scene(task)
    ids = ENV_IDS[task]
    if task == ABI.TASK_FEEDING:
        from avr import reset as RS
        S = np.concatenate([RS.batch_reset_states(A, md, 1001, ids[:2], genders=GENDERS[:2])[0],
                            RS.batch_reset_states(A, md, 1001, ids[2:], genders=GENDERS[2:], impairment='tremor')[0]])
    elif task == ABI.TASK_SCRATCH:
        from avr import reset_scratch as RSS
        S = RSS.batch_reset_states(A, md, 1001, ids, genders=GENDERS, impairment='tremor', attempts=8, iters=60)[0]
    else:
        from avr import reset_bedbath as RBB
        from oracle.oracle import Oracle

        def run(S0, frames):
            o = Oracle(md, len(S0), 'f64')
            o.set_threads(4)
            o.set_state(S0)
            o.settle(frames)
            return o.get_state()
        S = RBB.batch_reset_states(A, md, 1001, ids, genders=GENDERS, attempts=8, iters=60, settled=RBB.settled_arms(A, md, runner=run))[0]
    return np.ascontiguousarray(S, np.float32)


CASES = ('world', 'head')              # the cameras of every task's image tests


def case_env(task, name):
    """The env each case renders, a man and a woman per task: FeedingJaco's world camera env 1 (a woman)
    and its head camera env 2 (a man in the tremor env, whose head chain moves); the PR2 tasks' world
    camera env 0 (a man) and their head camera env 1 (a woman at the same reset draws)."""
    if task == ABI.TASK_FEEDING:
        return 1 if name == 'world' else 2
    return 0 if name == 'world' else 1


# The view of each task, found by search with the reference alone (the conditions of
# test_render_host.py: at most 25 % edge pixels, 20 non-edge pixels on every body kind).  An edge pixel's
# depth clause marks every surface turned more than about 27 degrees from the ray, at any resolution, so
# the view has to face the surfaces: it looks straight down on the tool from z = 4 m.  span: metres the
# image height covers at the tool's level; dens: pixels per metre there; aim: how far the centre moves
# from the tool towards the nearest human body (share of that distance); clip: the height below which
# `far` cuts the scene (the PR2's base and the wheelchair's wheels are all slopes; None: far = 10);
# aspect: width / height.
VIEW = {ABI.TASK_FEEDING: dict(span=0.30, dens=300, aim=0.3, clip=None, aspect=1.5),
        ABI.TASK_SCRATCH: dict(span=0.25, dens=240, aim=0.0, clip=0.5, aspect=2.5),
        ABI.TASK_BEDBATH: dict(span=0.25, dens=240, aim=0.0, clip=0.5, aspect=1.5)}
EYE_Z = 4.0
HEAD_TILT = 10.0


def tool_body(task):
    return int(scene(task)[1].desc.spoon_body)


def case_camera(task, name, poses):
    """The camera of case `name` for an env whose body poses [n_bodies, 7] are `poses` (the PR2's base,
    and with it the tool, stands somewhere else in every env, so the view is aimed per env):
      world  the task's VIEW as a world camera
      head   a camera riding on the head's body: the world view with its eye moved 10 degrees off the
             vertical, eye, target and up expressed in the head's frame at the time the camera is made
             (a camera on a mast on the head, which moves with the head from then on).  A head camera that looks forward
             sees every surface at a slope: 0.44 - 0.82 edge share in every variant searched.
    The tasks' GUI cameras (render.default_camera) come out at 0.91 - 0.94 edge share at 48 x 32, 72 x 48
    and 96 x 64 alike, which is why the cases do not use them."""
    A, md = scene(task)
    P = np.asarray(poses, np.float64)
    V = VIEW[task]
    tool, head = tool_body(task), RD.head_body(A, md)
    hb = np.nonzero(np.asarray(A['body_kind']) == ABI.BODY_HUMAN)[0]
    c = P[tool, :3]
    near = P[hb][np.argmin(np.linalg.norm(P[hb, :2] - c[:2], axis=1)), :2]
    x, y = c[:2] + V['aim'] * (near - c[:2])
    H = int(round(V['span'] * V['dens'] / 8)) * 8
    kw = dict(fov_y_deg=2 * np.degrees(np.arctan(V['span'] / 2 / (EYE_Z - c[2]))), width=int(H * V['aspect']), height=H,
              far=10.0 if V['clip'] is None else EYE_Z - V['clip'])
    eye, tgt, up = np.array([x, y, EYE_Z]), np.array([x, y, 0.0]), np.array([0.0, 1.0, 0.0])
    if name == 'world':
        return RD.Camera.world(eye, tgt, up, **kw)
    # the head case: the eye moved HEAD_TILT degrees off the vertical towards +x, about the point under
    # it at the tool's level (still within the slope the edge rule leaves to floor and lap), then
    # expressed in the head's frame
    tgt = np.array([x, y, c[2]])
    eye = np.array([x + (EYE_Z - c[2]) * np.tan(np.radians(HEAD_TILT)), y, EYE_Z])
    if V['clip'] is not None:
        kw['far'] = (EYE_Z - V['clip']) / np.cos(np.radians(HEAD_TILT))
    qc = np.array([-P[head, 3], -P[head, 4], -P[head, 5], P[head, 6]])
    return RD.Camera.on_body(head, _rot(qc, eye - P[head, :3]), _rot(qc, tgt - P[head, :3]), _rot(qc, up), **kw)


def _rot(q, v):
    u, w = q[:3], q[3]
    t = 2 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], a.dtype)


def robot_link_poses(A, q, base, dtype=np.float64):
    """COM frames [n_links, 7] of the compiled robot at joint vector q on base frame base [7]: the
    recursion of avr/reset.py robot_fk, in dtype arithmetic on inputs rounded to float32."""
    f = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(dtype)   # noqa: E731
    nl = int(A['n_links'])
    q, base = f(q), f(base)
    LP, LQ, out = np.zeros((nl, 3), dtype), np.zeros((nl, 4), dtype), np.zeros((nl, 7), dtype)
    for i in range(nl):
        p = int(A['rl_parent'][i])
        pp, pq = (base[:3], base[3:]) if p < 0 else (LP[p], LQ[p])
        tp, tq = pp + _rot(pq, f(A['rl_jpos'][i])), _qmul(pq, f(A['rl_jquat'][i]))
        ax, dof = f(A['rl_axis'][i]), int(A['rl_dof'][i])
        if A['rl_jtype'][i] == 1:
            h = dtype(0.5) * q[dof]
            tq = _qmul(tq, np.concatenate([ax * np.sin(h), [np.cos(h)]]).astype(dtype))
        elif A['rl_jtype'][i] == 2:
            tp = tp + _rot(tq, ax) * q[dof]
        LP[i], LQ[i] = tp, tq
        out[i, :3], out[i, 3:] = tp + _rot(tq, f(A['rl_com_pos'][i])), _qmul(tq, f(A['rl_com_quat'][i]))
    return out


def host_body_poses(task, row, dtype=np.float64):
    """[n_bodies, 7]: the body COM frames a state row gives (include/avr.h): ROBOT links by forward
    kinematics on S_Q, FREE bodies from S_FREE, HUMAN slots from S_HUMAN as the row holds them, STATIC
    bodies from st_pose, RSTATIC bodies at the robot base."""
    A, md = scene(task)
    L = md.layout
    row = np.asarray(row, np.float64)
    base = np.asarray(A['robot_base'], np.float64) if task == ABI.TASK_FEEDING else row[L.S_RBASE:L.S_RBASE + 7]
    links = robot_link_poses(A, row[L.S_Q:L.S_Q + int(A['n_dof'])], base, dtype)
    out = np.zeros((len(A['body_kind']), 7), dtype)
    for b, (k, i) in enumerate(zip(A['body_kind'], A['body_index'])):
        if k == ABI.BODY_ROBOT:
            out[b] = links[i]
        elif k == ABI.BODY_FREE:
            out[b] = row[L.S_FREE + ABI.FB_WORDS * i:L.S_FREE + ABI.FB_WORDS * i + 7]
        elif k == ABI.BODY_STATIC:
            out[b] = np.asarray(A['st_pose'], np.float64).reshape(-1, 7)[i]
        elif k == ABI.BODY_RSTATIC:
            out[b] = base
        else:
            out[b] = row[L.S_HUMAN + 7 * i:L.S_HUMAN + 7 * i + 7]
    return out


def chain_slot_poses(task, row, dtype=np.float64):
    """{human slot: [7] frame} of the articulated human chain's links (FeedingJaco's head and neck under
    'tremor', the PR2 tasks' right arm) by forward kinematics on the chain's joint words of the state
    row, from the parent slot's pose in the row: joint origin hc_jpos of the env's gender in the parent
    link's frame, a turn about hc_axis, the link's frame being its COM frame; dtype arithmetic on inputs
    rounded to float32."""
    A, md = scene(task)
    L = md.layout
    f = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(dtype)   # noqa: E731
    row = np.asarray(row, np.float64)
    g, nd, n = int(row[L.S_TASK + L.T_GENDER]), int(A['n_dof']), int(A['hc_n'])
    ps = int(A['hc_parent_slot'])
    t = f(row[L.S_HUMAN + 7 * ps:L.S_HUMAN + 7 * ps + 7])
    tp, tq, out = t[:3], t[3:], {}
    for c in range(n):
        tp = tp + _rot(tq, f(A['hc_jpos'][g][c]))
        h = dtype(0.5) * f(row[L.S_Q + nd + c])
        tq = _qmul(tq, np.concatenate([f(A['hc_axis'][c]) * np.sin(h), [np.cos(h)]]).astype(dtype))
        if int(A['hc_slot'][c]) >= 0:
            out[int(A['hc_slot'][c])] = np.concatenate([tp, tq])
    return out


def kind_groups(A):
    """{group: bool [n_shapes]}: the shapes of robot (with robot-fixed), human, static and tool / free bodies."""
    bk = np.asarray(A['body_kind'])[np.asarray(A['shape_body'])]
    return {'robot': (bk == ABI.BODY_ROBOT) | (bk == ABI.BODY_RSTATIC), 'human': bk == ABI.BODY_HUMAN, 'static': bk == ABI.BODY_STATIC,
            'tool/free': bk == ABI.BODY_FREE}


def coverage(A, ids, keep):
    """{group: compared pixels}: the non-edge (keep) pixels whose hit shape belongs to each group."""
    G = kind_groups(A)
    hit = keep & (ids >= 0)
    return {g: int(m[ids[hit]].sum()) for g, m in G.items()}
