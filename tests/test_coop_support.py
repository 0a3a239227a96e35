"""AVR_COOP_WSUP=0|1: the wave-cooperative narrowphase (EPA for penetrating cores, the GJK reruns in
double, big hulls) takes a hull's support point either with the serial scans or wave-wide -- a hull
of at most 64 vertices one vertex per lane from registers, a larger table hull its cell's candidates
one per lane.  Both return the first strictly largest projection in vertex order, so no bit of any
query result, state, output or flag may differ between the two.

Query hook: avr_narrowphase_query on two one-env handles per task.  Per class of hull (at most 8
vertices; 9 to 63; exactly 64; the smallest above 64; the largest) one hull, on side A and on side
B, against a hull, a box and a capsule; half the poses with the cores overlapping (EPA), half 0 to
3 mm apart (GJK only), classified with the fp64 oracle.

Step test: the switch off against on over two gym steps with a masked reset in between.  The
library places env-group boundaries on multiples of 32 envs, so the FeedingJaco case runs 64 envs in
two groups of 32 (the first 32 and the second 32 each hold both DoF counts)."""
import os

import numpy as np
import pytest

from avr import _abi as ABI
from avr import geom as G

pytestmark = pytest.mark.gpu

VAR = 'AVR_COOP_WSUP'
KEYS = (VAR, 'AVR_NP_HOT', 'AVR_PAIRS_FLAT', 'AVR_DYN_SPLIT', 'AVR_ENV_GROUPS', 'AVR_B4_GLOBAL', 'AVR_GRAPH', 'AVR_TAB_MIN_NV')
OFF, ON = 0, 1
SPHERE, CAPSULE, BOX, HULL = 0, 1, 2, 3
POSES = 25                      # per (class, partner, side, regime): 400 queries per class
MIN_PER_CLASS = 40              # penetrating, and separated-in-range, results a class must hold
THR = 0.02


def make_sim(md, n, v, groups=None):
    """A handle created with AVR_COOP_WSUP = v (and AVR_ENV_GROUPS) set; the environment is put back."""
    from avr import _lib
    old = {k: os.environ.pop(k, None) for k in KEYS}
    os.environ[VAR] = str(v)
    if groups:
        os.environ['AVR_ENV_GROUPS'] = str(groups)
    try:
        sim = _lib.Sim(md, n)
    finally:
        for k in KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    assert sim.coop_wsup() == v
    return sim


def bits(x):
    """Bit patterns: equality that also holds a NaN to its payload and tells -0 from +0."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_outs(o1, o2):
    return len(o1) == len(o2) and all(len(a) == len(b) and all(same(x, y) for x, y in zip(a, b)) for a, b in zip(o1, o2))


# ---------------------------------------------------------------------------- query hook
def hull_classes(A):
    """{class name: shape index}: one hull per class of vertex count present in the scene."""
    sk = np.asarray(A['shape_kind'])
    nv = np.asarray(A['shape_hull']).reshape(-1, 4)[:, 1]
    hulls = np.where(sk == HULL)[0]
    pick = {}
    small = hulls[nv[hulls] <= 8]
    mid = hulls[(nv[hulls] > 8) & (nv[hulls] < 64)]
    big = hulls[nv[hulls] > 64]
    if len(small):
        pick['le8'] = int(small[np.argmax(nv[small])])
    if len(mid):
        pick['9to63'] = int(mid[np.argsort(nv[mid], kind='stable')[len(mid) // 2]])
    if np.any(nv[hulls] == 64):
        pick['64'] = int(hulls[nv[hulls] == 64][0])
    if len(big):
        pick['above64'] = int(big[np.argmin(nv[big])])
        pick['largest'] = int(big[np.argmax(nv[big])])
    return pick, nv


def partners(A, nv, h):
    """A hull of 9 to 63 vertices and one above 64 (neither is h: both table sides and both resident
    sides meet), a box and a capsule."""
    sk = np.asarray(A['shape_kind'])
    mid = [int(s) for s in np.where(sk == HULL)[0] if 8 < nv[s] < 64 and s != h]
    big = [int(s) for s in np.where(sk == HULL)[0] if nv[s] > 64 and s != h]
    return [mid[len(mid) // 3], big[len(big) // 2], int(np.where(sk == BOX)[0][0]), int(np.where(sk == CAPSULE)[0][0])]


def centre(A, s):
    """An interior point of shape s's core, shape frame: a hull's vertex mean, else the origin."""
    if int(A['shape_kind'][s]) != HULL:
        return np.zeros(3)
    v0, n = np.asarray(A['shape_hull']).reshape(-1, 4)[s][:2]
    return np.asarray(A['hull_verts'], np.float64).reshape(-1, 3)[v0:v0 + n].mean(0)


def inradius(A, s):
    """A length well inside shape s's core around centre(): a share of its smallest AABB half extent
    (a capsule's core is its segment: its radius does not count)."""
    h = np.asarray(A['shape_aabb'][s][3:6], np.float64)
    if int(A['shape_kind'][s]) == CAPSULE:
        return 0.0
    return 0.25 * float(h.min())


def place(A, sa, sb, qa, qb, off):
    """Body poses (14 words) with shape sa's centre at shape sb's centre + off (world)."""
    pb = np.array([0.3, 0.1, 0.9])
    Pb, Qb = G.tf_mul(pb, qb, A['shape_pose'][sb][:3], A['shape_pose'][sb][3:])
    cb = Pb + G.quat_rotate(Qb, centre(A, sb))
    _, Qa = G.tf_mul(np.zeros(3), qa, A['shape_pose'][sa][:3], A['shape_pose'][sa][3:])
    Pa = cb + off - G.quat_rotate(Qa, centre(A, sa))
    pa = Pa - G.quat_rotate(qa, A['shape_pose'][sa][:3])
    return np.concatenate([pa, qa, pb, qb])


def build_queries(A, md, seed):
    """(pairs, poses, class of each query, regime of each query: 0 overlapping cores, 1 apart)."""
    from oracle.oracle import Oracle
    o = Oracle(md, 1, 'f64')
    rng = np.random.default_rng(seed)
    classes, nv = hull_classes(A)
    pairs, X, cls, reg = [], [], [], []
    for ci, (name, h) in enumerate(classes.items()):
        for p in partners(A, nv, h):
            for sa, sb in ((h, p), (p, h)):
                for k in range(2 * POSES):
                    qa = G.quat_normalize(G.quat_axis_angle(rng.standard_normal(3), rng.uniform(0, np.pi)))
                    qb = G.quat_normalize(G.quat_axis_angle(rng.standard_normal(3), rng.uniform(0, np.pi)))
                    u = rng.standard_normal(3)
                    u /= np.linalg.norm(u)
                    if k < POSES:       # the cores overlap: the centres closer than either core is thick
                        x = place(A, sa, sb, qa, qb, u * rng.uniform(0, 1) * max(inradius(A, sa), inradius(A, sb)))
                    else:               # approached along u, then moved along the contact normal to 0 .. 3 mm
                        reach = 0.5 * (np.linalg.norm(A['shape_aabb'][sa][3:6]) + np.linalg.norm(A['shape_aabb'][sb][3:6])) + 0.05
                        x = place(A, sa, sb, qa, qb, u * 2.0 * reach)
                        r, out = o.narrowphase(sa, x[:7], sb, x[7:], 10.0)
                        assert r, 'oracle found no closest points for the approach pose'
                        x[:3] += out[:3] * (rng.uniform(0, 0.003) - out[6])
                    pairs.append((sa, sb)); X.append(x); cls.append(ci); reg.append(int(k >= POSES))
    return np.array(pairs, np.int32), np.array(X), np.array(cls), np.array(reg), list(classes.items()), nv


@pytest.mark.parametrize('task', [0, 1, 2], ids=['FeedingJaco', 'ScratchItchPR2', 'BedBathingPR2'])
def test_query_hook_switch_off_and_on_agree(task, oracle_built):
    from oracle.oracle import Oracle
    A = ABI.load_scene(task)
    md = ABI.ModelDesc(A)
    pairs, X, cls, reg, classes, nv = build_queries(A, md, 31 + task)
    names = [n for n, _ in classes]
    assert {'le8', '9to63', 'above64', 'largest'} <= set(names)
    # classified by the fp64 oracle: cores overlapping (distance below minus both margins: EPA) or
    # a contact with the cores apart (GJK only)
    o = Oracle(md, 1, 'f64')
    mg = np.asarray(A['shape_margin'], np.float64)
    pen = np.zeros(len(pairs), bool)
    sep = np.zeros(len(pairs), bool)
    for k, (sa, sb) in enumerate(pairs):
        r, out = o.narrowphase(int(sa), X[k, :7], int(sb), X[k, 7:], THR)
        pen[k] = bool(r) and out[6] < -(mg[sa] + mg[sb])
        sep[k] = bool(r) and out[6] >= -(mg[sa] + mg[sb])
    res = []
    for v in (OFF, ON):
        sim = make_sim(md, 1, v)
        try:
            res.append(sim.narrowphase(pairs, X, THR))
        finally:
            sim.close()
    g0, g1 = res
    for ci, (name, h) in enumerate(classes):
        m = cls == ci
        print('%s: hull %d (%d vertices), %d queries, oracle: %d penetrating, %d separated in range; GPU contacts %d'
              % (name, h, nv[h], m.sum(), (pen & m).sum(), (sep & m).sum(), int((g0[m, 0] == 1).sum())))
        assert (pen & m).sum() >= MIN_PER_CLASS and (sep & m).sum() >= MIN_PER_CLASS
    diff = np.where(np.any(bits(g0) != bits(g1), axis=1))[0]
    print('%d queries, %d differ' % (len(pairs), len(diff)))
    for k in diff[:8]:
        print('  query %d pair %s class %s regime %d: off %s on %s' % (k, pairs[k].tolist(), names[cls[k]], reg[k], g0[k].tolist(), g1[k].tolist()))
    assert len(diff) == 0


# ---------------------------------------------------------------------------- steps
def _ncp(Gs, L=ABI):
    return Gs[:, L.S_TASK + L.T_NCP]


def _min_dist(Gs, L=ABI):
    """Smallest contact distance held in each env's pool (+inf without a point)."""
    n = _ncp(Gs, L).astype(int)
    d = np.full(len(Gs), np.inf)
    for e in range(len(Gs)):
        if n[e] > 0:
            d[e] = Gs[e, L.S_CP:L.S_CP + ABI.CP_WORDS * n[e]].reshape(n[e], ABI.CP_WORDS)[:, ABI.CP_DIST].min()
    return d


def test_feeding_steps_from_raw_reset_states_agree(scene):
    """Raw reset states (the food dropped into the spoon penetrates there), two gym steps, every third
    env put back to its raw state in between."""
    from avr import _lib, reset as RS
    A, md = scene
    raw = np.concatenate([RS.batch_reset_states_fast(A, md, 1001, list(ids), impairment=imp)[0]
                          for ids, imp in ((range(0, 20), 'random'), (range(20, 32), 'tremor'), (range(32, 52), 'random'), (range(52, 64), 'tremor'))]).astype(np.float32)
    n = len(raw)
    mask = np.zeros(n, np.uint8); mask[::3] = 1
    res = []
    for v in (OFF, ON):
        sim = make_sim(md, n, v, groups=2)
        assert sim.env_groups() == 2
        sim.set_state(raw)
        states, outs = [], []
        for k in range(2):
            if k == 1:
                sim.set_state_masked(mask, raw)
            outs.append(sim.step(_lib.random_actions(1001, np.arange(n), k)))
            states.append(sim.get_state())
        res.append((states, outs, sim.get_flags()))
        sim.close()
    (G0, o0, f0), (G1, o1, f1) = res
    for g in G0:
        d = _min_dist(g)
        print('contact points: mean %.1f, envs with one %d of %d; envs with a contact below 0: %d, smallest %.4g'
              % (_ncp(g).mean(), np.count_nonzero(_ncp(g) > 0), n, np.count_nonzero(d < 0), d.min()))
        assert np.all(_ncp(g) > 0) and np.any(d < 0)         # contacts everywhere, and a penetrating one: an EPA was reached
    assert not np.any(f0 & _lib.FLAGS_FAULT_MASK)
    assert np.array_equal(f0, f1)
    assert all(same(a, b) for a, b in zip(G0, G1))
    assert same_outs(o0, o1)


def _pr2_states(task, n):
    """n reset states of a PR2 task with the tool pressed 2 mm into the arm."""
    from avr import _lib
    A = ABI.load_scene(task)
    md = ABI.ModelDesc(A)
    sim = _lib.Sim(md, 1)
    try:
        if task == ABI.TASK_BEDBATH:
            import bedbath_util as U
            from avr import reset_bedbath as RBB
            S, _ = RBB.batch_reset_states(A, md, 1001, list(range(n)), sim=sim, device=0)
            C, _ = U.wipe_states(A, md, S, strict=False)
        else:
            import scratch_util as U
            from avr import reset_scratch as RSS
            S, meta = RSS.batch_reset_states(A, md, 1001, list(range(n)), sim=sim)
            C = U.contact_states(A, md, S, meta)
    finally:
        sim.close()
    return md, S.astype(np.float32), C.astype(np.float32)


@pytest.mark.parametrize('task', ['scratch', 'bedbath'])
def test_pr2_steps_from_pressed_tool_states_agree(task):
    """8 pressed-tool states of each PR2 task: two gym steps with every third env put back in between;
    BedBathing also through its closest-distance query (the step's queue, and a queue of 0 words, which
    sends every stalled pair to the stall kernel's rerun)."""
    from avr import _lib
    md, S0, C = _pr2_states(ABI.TASK_SCRATCH if task == 'scratch' else ABI.TASK_BEDBATH, 8)
    assert len(C) > 0
    L = ABI.SI if task == 'scratch' else ABI.BB
    n = len(C)
    mask = np.zeros(n, np.uint8); mask[::3] = 1
    res = []
    for v in (OFF, ON):
        sim = make_sim(md, n, v)
        sim.set_state(C)
        states, outs, close = [], [], []
        for k in range(2):
            if k == 1:
                sim.set_state_masked(mask, C)
            if task == 'bedbath':
                close += [sim.bb_closest_query(), sim.bb_closest_query(0)]
            outs.append(sim.step(_lib.random_actions(1001, np.arange(n), k) * 0.5))
            states.append(sim.get_state())
        res.append((states, outs, sim.get_flags(), close))
        sim.close()
    (G0, o0, f0, c0), (G1, o1, f1, c1) = res
    for g in G0:
        d = _min_dist(g, L)
        print(task, 'contact points', _ncp(g, L).astype(int).tolist(), 'smallest distance %.4g' % d.min())
        assert _ncp(g, L).max() > 0 and np.any(d < 0)
    assert np.array_equal(f0, f1)
    assert all(same(a, b) for a, b in zip(G0, G1))
    assert same_outs(o0, o1)
    assert len(c0) == len(c1) and all(same(a, b) for a, b in zip(c0, c1))
