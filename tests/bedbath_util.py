"""BedBathingPR2 test helpers: wiping contact states -- the PR2's arm solved by IK (the reset's DLS
restatement) so that the cloth (tool link 1) lies on an upward-facing upper-arm target, pressed in
by `depth`, its face along the arm's surface normal there."""
import numpy as np

from avr import _abi as ABI
from avr import geom as G
from avr import reset_bedbath as RBB
from avr import reset_scratch as RSS

BB = ABI.BB


def reset_states8(A, md):
    """The 8 reset states of test_bedbath.py's `states` fixture (the arm settle on the fp64 oracle)."""
    from oracle.oracle import Oracle

    def run(S, frames):
        o = Oracle(md, len(S), 'f64')
        o.set_threads(4)
        o.set_state(S)
        o.settle(frames)
        return o.get_state()
    settled = RBB.settled_arms(A, md, runner=run)
    return RBB.batch_reset_states(A, md, 1001, list(range(8)), attempts=12, iters=80, settled=settled)[0]


def near_contact_states(A, md, S, n, seed, lo, hi):
    """n BedBathing states with the wiper lo..hi (m) from the person: the rows of S, cycled, with
    the wiper (S_FREE's pose) re-placed -- a random wiper shape and a random human shape of the
    env's gender (any kind), a random wiper orientation, the wiper shape's centre at the human
    shape's centre + u (|human shape's AABB half extent| / 4 + |wiper shape's| / 2) along a random
    unit u, then the wiper moved along the fp64 oracle's normal of that pair to a distance drawn
    from [lo, hi].  Rounded to fp32 (what the device holds); returned as float64."""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(seed)
    S = np.asarray(S, np.float64)
    tb = int(A['task_tool_body'])
    ts0, nts = int(A['body_shape_start'][tb]), int(A['body_shape_count'][tb])
    sbod, sgen = np.asarray(A['shape_body']), np.asarray(A['shape_gender'])
    hum = np.nonzero(np.asarray(A['body_kind'])[sbod] == ABI.BODY_HUMAN)[0]
    cand = [hum[(sgen[hum] < 0) | (sgen[hum] == g)] for g in (0, 1)]
    ext = np.linalg.norm(np.asarray(A['shape_aabb'])[:, 3:6], axis=1)
    o = Oracle(md, 1, 'f64')
    out = np.zeros((n, S.shape[1]))
    for k in range(n):
        st = S[k % len(S)].copy()
        g = int(st[BB.S_TASK + BB.T_GENDER])
        sa, sb = ts0 + int(rng.integers(nts)), int(rng.choice(cand[g]))
        qa = G.quat_axis_angle(rng.standard_normal(3), rng.uniform(0, np.pi))
        qa = qa / np.linalg.norm(qa)
        slot = int(A['body_index'][sbod[sb]])
        hp = st[BB.S_HUMAN + 7 * slot:BB.S_HUMAN + 7 * slot + 7]
        cb = hp[:3] + G.quat_rotate(hp[3:], A['shape_pose'][sb][:3])
        u = rng.standard_normal(3)
        u /= np.linalg.norm(u)
        ca = cb + u * (0.25 * ext[sb] + 0.5 * ext[sa])
        pa = ca - G.quat_rotate(qa, A['shape_pose'][sa][:3])
        d = rng.uniform(lo, hi)
        r, o7 = o.narrowphase(sa, np.concatenate([pa, qa]), sb, hp, 4.0)
        if r:
            pa = pa + o7[:3] * (d - o7[6])
        st[BB.S_FREE:BB.S_FREE + 3] = pa
        st[BB.S_FREE + 3:BB.S_FREE + 7] = qa
        out[k] = st
    o.close()
    return out.astype(np.float32).astype(np.float64)


def closest_labels(md, S, chunk=1000):
    """Per state of S, the oracle's closest tool-human distance (bb_closest): dict of
    stall (the fp32 oracle's stalled pairs: the stats()[5] delta around the query), d64 (fp64
    oracle), d32 (fp32 oracle, the lane GJK's stall rule on, as the kernel), d32_plain (the rule
    off), stall64 (the fp64 oracle's stalled pairs, all states together)."""
    from oracle.oracle import Oracle
    n = len(S)
    L = dict(stall=np.zeros(n, np.int64), d64=np.zeros(n), d32=np.zeros(n), d32_plain=np.zeros(n), stall64=0)
    for c0 in range(0, n, chunk):
        X = S[c0:c0 + chunk]
        o64, o32 = Oracle(md, len(X), 'f64'), Oracle(md, len(X), 'f32')
        o64.set_state(X)
        o32.set_state(X)
        s0 = o64.stats()[5]
        for e in range(len(X)):
            L['d64'][c0 + e] = o64.bb_closest(e)
        L['stall64'] += int(o64.stats()[5] - s0)
        for e in range(len(X)):
            s0 = o32.stats()[5]
            L['d32'][c0 + e] = o32.bb_closest(e)
            L['stall'][c0 + e] = o32.stats()[5] - s0
        o32.set_np_plain(True)
        for e in range(len(X)):
            L['d32_plain'][c0 + e] = o32.bb_closest(e)
        o64.close()
        o32.close()
    return L


def step_prediction(A, md, P, chunk=1024):
    """What the fp32 oracle predicts for one zero-action step from the states P: dict of G (its
    post-step states, rounded to fp32), free (no force on the person: info[:, 0] == 0), stall (the
    stalled pairs of bb_closest on G) and gap (for the force-free envs with a stall: how far the
    closest stalled pair lies below the closest other pair -- what the kernel's rerun takes off
    the lane and cooperative pairs' minimum; 0 elsewhere)."""
    from oracle.oracle import Oracle
    n = len(P)
    tb = int(A['task_tool_body'])
    ts0, nts = int(A['body_shape_start'][tb]), int(A['body_shape_count'][tb])
    sbod, sgen = np.asarray(A['shape_body']), np.asarray(A['shape_gender'])
    hum = np.nonzero(np.asarray(A['body_kind'])[sbod] == ABI.BODY_HUMAN)[0]
    R = dict(G=np.zeros_like(P), free=np.zeros(n, bool), stall=np.zeros(n, np.int64), gap=np.zeros(n))
    o1 = Oracle(md, 1, 'f32')
    for c0 in range(0, n, chunk):
        X = P[c0:c0 + chunk]
        o = Oracle(md, len(X), 'f32')
        o.set_threads(4)
        o.set_state(X)
        _, _, _, info = o.step(np.zeros((len(X), 7), np.float32))
        Gs = o.get_state().astype(np.float32).astype(np.float64)
        o.set_state(Gs)
        R['G'][c0:c0 + chunk] = Gs
        R['free'][c0:c0 + chunk] = info[:, 0] == 0
        for e in range(len(X)):
            s0 = o.stats()[5]
            o.bb_closest(e)
            R['stall'][c0 + e] = o.stats()[5] - s0
        o.close()
        for e in np.nonzero(R['free'][c0:c0 + chunk] & (R['stall'][c0:c0 + chunk] > 0))[0]:
            st = Gs[e]
            g = int(st[BB.S_TASK + BB.T_GENDER])
            tp = st[BB.S_FREE:BB.S_FREE + 7]
            d_st, d_ot = [], [float(md.desc.closest_distance)]
            for sb in hum[(sgen[hum] < 0) | (sgen[hum] == g)]:
                slot = int(A['body_index'][sbod[sb]])
                hp = st[BB.S_HUMAN + 7 * slot:BB.S_HUMAN + 7 * slot + 7]
                for sa in range(ts0, ts0 + nts):
                    s0 = o1.stats()[5]
                    r, o7 = o1.narrowphase(sa, tp, int(sb), hp, float(md.desc.closest_distance))
                    if r:
                        (d_st if o1.stats()[5] > s0 else d_ot).append(o7[6])
            R['gap'][c0 + e] = max(min(d_ot) - min(d_st + d_ot), 0.0)
    o1.close()
    return R


def scan_step_seeds(A, md, S, seeds, block=8, lo=0.001, hi=0.020):
    """The seeds whose block of near-contact states holds, by step_prediction, a force-free env
    whose closest pair is stalled after the step (how tests/golden/bedbath_closest_step_seeds.json
    was chosen, with S = reset_states8(); about 2500 states a second and core)."""
    keep = []
    for s in seeds:
        R = step_prediction(A, md, near_contact_states(A, md, S, block, s, lo, hi))
        if (R['free'] & (R['gap'] > 1e-4)).any():
            keep.append(s)
    return keep


def _frame_z(n, x_hint):
    """Rotation (quaternion) whose z axis is n, x axis the projection of x_hint."""
    z = n / np.linalg.norm(n)
    x = x_hint - np.dot(x_hint, z) * z
    if np.linalg.norm(x) < 1e-6:
        x = np.cross(z, [1.0, 0, 0]) if abs(z[0]) < 0.9 else np.cross(z, [0, 1.0, 0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(np.stack([x, y, z], 1)).as_quat()


def wipe_states(A, md, S, depth=0.002, tries=12, strict=True):
    """Copy of S with every env's left arm re-solved so the cloth presses on an upper-arm target;
    returns (states, target index per env).  strict=False drops the envs whose base pose reaches
    none of the `tries` upward-facing targets (strict: an assertion)."""
    S = S.copy()
    nd = int(A['n_dof'])
    arm = np.array(md.arm_dofs)
    lo = np.array([md.desc.arm_lower[i] if md.desc.arm_lower[i] > -1e9 else -2 * np.pi for i in range(len(arm))])
    hi = np.array([md.desc.arm_upper[i] if md.desc.arm_upper[i] < 1e9 else 2 * np.pi for i in range(len(arm))])
    link = int(A['task_tool_link'])
    tip, piv = A['task_tool_tip'], A['task_tool_pivot']
    ks, keep = [], []
    for e in range(len(S)):
        st = S[e]
        g = int(st[BB.S_TASK + BB.T_GENDER])
        ls = int(A['bb_limb_slots'][0])
        lp = st[BB.S_HUMAN + 7 * ls:BB.S_HUMAN + 7 * ls + 7]
        R = G.quat_to_mat(lp[3:])
        nu = int(A['bb_ntgt'][g][0])
        T = A['bb_targets'][g][:nu, :3]
        nrm = (R @ np.concatenate([T[:, :2], np.zeros((nu, 1))], 1).T).T
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        order = np.argsort(-nrm[:, 2])            # facing up first
        bp, bq = st[BB.S_RBASE:BB.S_RBASE + 3][None], st[BB.S_RBASE + 3:BB.S_RBASE + 7][None]
        tb = st[BB.S_FREE:BB.S_FREE + 7]
        xh = G.quat_rotate(tb[3:], [1.0, 0, 0])
        best = None
        for k in order[:tries]:
            tw = lp[:3] + R @ T[k]
            n = nrm[k]
            cq = _frame_z(n, xh)
            cc = tw + n * (0.0025 - depth)
            body_p = cc - G.quat_rotate(cq, tip)
            tp = body_p + G.quat_rotate(cq, piv)
            Q0 = st[BB.S_Q:BB.S_Q + nd][None].copy()
            Q, CP, CQ, _, _ = RSS.ik_dls(A, link, Q0, bp, bq, tp[None], cq[None], arm, lo, hi, 400)
            pe = np.linalg.norm(CP[0, link] - tp)
            qe = min(np.linalg.norm(CQ[0, link] - cq), np.linalg.norm(CQ[0, link] + cq))
            if pe < 1e-3 and qe < 1e-2:
                best = (k, Q[0], CP[0, link], CQ[0, link])
                break
        if best is None and not strict:
            continue
        assert best is not None, 'env %d: no upper-arm target reachable' % e
        keep.append(e)
        k, q, cp, cq = best
        st[BB.S_Q:BB.S_Q + nd] = q
        st[BB.S_QD:BB.S_QD + nd] = 0
        for d in arm:
            st[BB.S_QTGT + d] = q[d]
        p, qq = RBB._tool_pose(A, cp, cq)
        st[BB.S_FREE:BB.S_FREE + 3] = p
        st[BB.S_FREE + 3:BB.S_FREE + 7] = qq
        st[BB.S_FREE + 7:BB.S_FREE + 13] = 0
        ks.append(int(k))
    return S[keep], ks
