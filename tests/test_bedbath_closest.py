"""BedBathing's closest-distance query where the fp32 lane GJK stalls: bb_closest's stalled-pair
queue in the env workspace and its rerun with the double simplex solve (avr_bb_stall_kernel,
csrc/avr_glue_bedbath.hip), through include/avr.h avr_bb_closest_query -- the step's own code on
the handle's state -- and through the step's reward, against the fp64 oracle's bb_closest.

Inputs: 8000 reset states with the wiper re-placed -1..20 mm from a random human shape
(bedbath_util.near_contact_states, seed 7).  The CPU test below pins what makes them a test of
the queue: the fp32 oracle (which restates the stall rule) stalls on 203 of them and is then
within 1.4e-7 m of fp64 on every stalled state, whereas without the rule (Oracle.set_np_plain) 32
stalled states are off by more than 1e-5 m, 16 by more than 2e-3 m, the largest 2.0e-2 m.  A rerun
that is dropped, reads a wrong pair key or another env's queue shows at that size; a miss is
1e-5 m (test_narrowphase_pairs._near_bad's distance threshold).
"""
import json
import os

import numpy as np
import pytest

from avr import _abi as ABI

import bedbath_util as U

BB = ABI.BB
N_POOL, E = 8000, 8192
MISS = 1e-5

# The step test's 4096 envs: 512 blocks of 8 near-contact states, 1..20 mm (near_contact_states
# with the seeds of tests/golden/bedbath_closest_step_seeds.json).  One zero-action step drags the
# wiper back to the gripper (16 cm at the median), so few post-step states are still near the
# person: the seeds are the first 512 of range(262144) for which the fp32 oracle's step
# (bedbath_util.step_prediction) leaves a force-free env whose closest pair stalls (gap > 1e-4 m;
# bedbath_util.scan_step_seeds -- about 1 state in 3800); test_step_pool_prediction holds that.
STEP_BLOCK = 8
with open(os.path.join(os.path.dirname(__file__), 'golden', 'bedbath_closest_step_seeds.json')) as _f:
    STEP_SEEDS = json.load(_f)['seeds']


@pytest.fixture(scope='module')
def bb():
    A = ABI.load_scene(ABI.TASK_BEDBATH)
    return A, ABI.ModelDesc(A)


@pytest.fixture(scope='module')
def reset8(bb, oracle_built):
    return U.reset_states8(*bb)


@pytest.fixture(scope='module')
def pool(bb, reset8):
    """(states (8000, words) float64 holding fp32 values, oracle labels)"""
    A, md = bb
    P = U.near_contact_states(A, md, reset8, N_POOL, 7, -0.001, 0.020)
    return P, U.closest_labels(md, P)


@pytest.fixture(scope='module')
def step_pool(bb, reset8):
    A, md = bb
    return np.concatenate([U.near_contact_states(A, md, reset8, STEP_BLOCK, s, 0.001, 0.020) for s in STEP_SEEDS])


def _padded(P):
    return np.concatenate([P, P[:E - len(P)]]).astype(np.float32)


def _poisson_ok(n_g, n_32):
    """the project's rule for two independent fp32 realisations (test_narrowphase_pairs.py)"""
    return n_g <= n_32 + 3.0 * np.sqrt(max(n_g + n_32, 1))


# ------------------------------------------------------------------ CPU: the inputs have teeth
def test_pool_has_teeth(pool):
    """The conditions that keep the GPU tests honest (measured, seed 7: 203 stalled states, 6 of
    them with two stalled pairs; with the rule 1 state beyond 1e-5 of fp64 -- 6.3e-5, not stalled;
    without it 33, 32 of them stalled, 16 beyond 2e-3, the largest 2.04e-2; fp64 stalls: 0)."""
    P, L = pool
    st = L['stall'] > 0
    e, ep = np.abs(L['d32'] - L['d64']), np.abs(L['d32_plain'] - L['d64'])
    print('stalled states %d (two pairs: %d), with the rule: misses %d (stalled %d), max on stalled %.3g; without: misses %d (stalled %d), '
          '> 2e-3 on stalled %d, max %.3g; fp64 stalls %d'
          % (st.sum(), (L['stall'] >= 2).sum(), (e > MISS).sum(), ((e > MISS) & st).sum(), e[st].max(), (ep > MISS).sum(), ((ep > MISS) & st).sum(),
             ((ep > 2e-3) & st).sum(), ep.max(), L['stall64']))
    assert st.sum() >= 100
    assert (e > MISS).sum() <= 3 and not ((e > MISS) & st).any()
    assert ((ep > MISS) & st).sum() >= 20 and ((ep > 2e-3) & st).sum() >= 8
    assert L['stall64'] == 0
    assert (L['stall'] >= 2).sum() >= 2            # the capacity test's cap 1 needs an env with two stalled pairs


def test_step_pool_prediction(bb, step_pool):
    """The step test's pool, by the fp32 oracle's step: at least 3 in 4 envs stay force-free, and
    every block of 8 holds a force-free env that ends the step with its closest pair stalled: 512
    and more of 4096 (measured: 512, 3234 envs force-free).  The GPU test asks for 5: the GPU
    stalls on other states than the oracle for the most part -- a stall is an event of the fp32
    arithmetic, and the kernel contracts into FMAs -- so about 1 predicted env in 15 is one on the
    GPU (measured: 33 of 512)."""
    A, md = bb
    assert len(step_pool) == 4096
    R = U.step_prediction(A, md, step_pool)
    teeth = R['free'] & (R['gap'] > 1e-4)
    print('fp32 oracle step: force-free %d of %d, stalled after the step %d, force-free with the closest pair stalled %d'
          % (R['free'].sum(), len(step_pool), (R['stall'] > 0).sum(), teeth.sum()))
    assert R['free'].mean() >= 0.75
    assert teeth.reshape(-1, STEP_BLOCK).any(1).all()


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def sim_q(bb):
    from avr import _lib
    sim = _lib.Sim(bb[1], E)
    yield sim
    sim.close()


@pytest.mark.gpu
def test_gpu_query_matches_fp64_oracle(sim_q, pool):
    """avr_bb_closest_query on the 8000 pool states against the fp64 oracle: misses (> 1e-5 m)
    at most 0.4 % and no more than the fp32 oracle's within Poisson noise; the envs that queued a
    stalled pair are as many as the fp32 oracle's stalled states within 3 sqrt(n), none of them a
    miss, and on at least 10 of them the rerun demonstrably mattered (it lowered the lane and
    cooperative pairs' minimum by > 1e-4 m, or the fp32 oracle without the rule is off by > 1e-4 m).
    Measured (MI355X): 0 GPU misses (fp32 oracle 1), largest error 2.3e-7 m; 237 envs queued 243
    pairs (the oracle stalls on 203 states, 36 of them common: two fp32 realisations), largest
    error on them 1.2e-7 m; on 40 the rerun lowered the minimum by > 1e-4 m, by up to 5.0e-2 m."""
    P, L = pool
    sim_q.set_state(_padded(P))
    out = sim_q.bb_closest_query().astype(np.float64)[:N_POOL]
    err, e32, ep = np.abs(out[:, 0] - L['d64']), np.abs(L['d32'] - L['d64']), np.abs(L['d32_plain'] - L['d64'])
    n_g, n_32 = int((err > MISS).sum()), int((e32 > MISS).sum())
    queued = out[:, 1] > 0
    n_q, n_st = int(queued.sum()), int((L['stall'] > 0).sum())
    teeth = queued & ((out[:, 2] - out[:, 0] > 1e-4) | (ep > 1e-4))
    print('query vs fp64: GPU misses %d (fp32 oracle %d) of %d, max err %.3g; queued envs %d (oracle stalled %d, both %d), queued pairs %d, '
          'max err on queued %.3g, misses on queued %d; teeth %d (rerun lowered the minimum by > 1e-4: %d, largest %.3g)'
          % (n_g, n_32, N_POOL, err.max(), n_q, n_st, int((queued & (L['stall'] > 0)).sum()), int(out[:, 1].sum()),
             err[queued].max() if n_q else -1, int((queued & (err > MISS)).sum()), int(teeth.sum()),
             int((queued & (out[:, 2] - out[:, 0] > 1e-4)).sum()), float((out[:, 2] - out[:, 0]).max())))
    assert np.all(np.isfinite(out)) and np.all(out[:, 3] == 0)
    assert n_g <= 0.004 * N_POOL and _poisson_ok(n_g, n_32), (n_g, n_32)
    assert n_q >= 50 and abs(n_q - n_st) <= 3.0 * np.sqrt(n_st), (n_q, n_st)
    assert not (queued & (err > MISS)).any()
    assert teeth.sum() >= 10


def _overflow_figures(sim, P, L, cap):
    """query at `cap` -> (out, overflowed pool envs, |d - d64| on the pool)"""
    sim.set_state(_padded(P))
    q = sim.bb_closest_query(cap)
    return q, (q[:N_POOL, 3] > 0), np.abs(q[:N_POOL, 0].astype(np.float64) - L['d64'])


@pytest.mark.gpu
def test_gpu_queue_capacity(sim_q, pool):
    """The queue's capacity (cap 0 and 1 for this call): the queue holds min(stalled, cap) pairs and
    the others are counted as overflow; envs within the capacity are bit-identical to the
    full-capacity result; at cap 1 some env has a queued and an overflowed pair.  The rerun finds
    the overflowed pairs again with the lane GJK and gives them the double solve too, so the final
    minimum is the full-capacity one bit for bit at every capacity, and the minimum before the rerun
    leaves them out (never below the final one where nothing else is closer).  Measured (MI355X):
    cap 0, 251 overflowed pairs in 245 envs; cap 1, 6 envs with a queued and an overflowed pair; the
    final minimum equal to the full-capacity one on all 8192 envs at both."""
    P, L = pool
    sim_q.set_state(_padded(P))
    full = sim_q.bb_closest_query()
    nstall = full[:, 1].astype(np.int64)
    assert np.all(full[:, 3] == 0) and nstall.max() >= 2
    for cap in (0, 1):
        q, o, err = _overflow_figures(sim_q, P, L, cap)
        nq, ovf = q[:, 1].astype(np.int64), q[:, 3].astype(np.int64)
        within = nstall <= cap
        print('cap %d: envs with overflow %d (pairs %d), with a queued and an overflowed pair %d; final minimum differs from full capacity on %d envs; '
              'minimum before the rerun above the final one on %d envs'
              % (cap, int((ovf > 0).sum()), int(ovf.sum()), int(((nq > 0) & (ovf > 0)).sum()), int((q[:, 0] != full[:, 0]).sum()),
                 int((q[:, 2] > q[:, 0]).sum())))
        assert np.array_equal(nq, np.minimum(nstall, cap)) and np.array_equal(ovf, nstall - nq)
        assert np.array_equal(q[within].view(np.uint32), full[within].view(np.uint32))
        if cap == 1:
            assert ((nq > 0) & (ovf > 0)).any()
        assert np.all(np.isfinite(q))
        assert np.array_equal(q[:, 0].view(np.uint32), full[:, 0].view(np.uint32))
        assert np.all(q[:, 2] >= q[:, 0])


@pytest.mark.gpu
def test_gpu_queue_overflow_accuracy_on_the_same_envs(sim_q, pool):
    """The overflowed envs against the fp64 oracle, with the plain fp32 oracle (no stall rule) on
    the same envs beside them: misses (> 1e-5 m) no more than the plain oracle's within Poisson
    noise (3 sqrt of the pooled count), and no env further off than twice the plain oracle's
    largest error over the pool (2.04e-2 m).  Measured (MI355X): cap 0, 0 misses on 237 envs (plain
    oracle 7), largest error 1.2e-7 m; cap 1, 0 misses on 6 envs (plain oracle 0), 1.2e-7 m.  (While the
    overflowed pairs took the fp32 cooperative GJK, cap 0 gave 38 misses on 237 envs against the
    plain oracle's 7 on the same envs, up to 2.04e-2 m off: the GPU and the oracle stall on
    different states for the most part, 36 common, so the GPU's own stalled pairs are where its
    fp32 GJK is inaccurate.  They now get the double solve in the stall kernel.)"""
    P, L = pool
    ep = np.abs(L['d32_plain'] - L['d64'])
    fig = []
    for cap in (0, 1):
        q, o, err = _overflow_figures(sim_q, P, L, cap)
        fig.append((cap, int((o & (err > MISS)).sum()), int((o & (ep > MISS)).sum()), float(err[o].max()), bool(np.all(np.isfinite(q)))))
        print('cap %d: overflowed pool envs %d vs fp64: misses %d (plain fp32 oracle on the same envs %d), max err %.3g (plain oracle over the pool %.3g)'
              % (cap, o.sum(), fig[-1][1], fig[-1][2], fig[-1][3], ep.max()))
    for cap, n_g, n_p, worst, finite in fig:
        assert finite
        assert _poisson_ok(n_g, n_p), (cap, n_g, n_p)
        assert worst <= 2.0 * ep.max(), (cap, worst)


def _qrot(q, v):
    """rotate v (3,) by the quaternions q (n, 4) xyzw, float64"""
    u, w = q[:, :3], q[:, 3:4]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


@pytest.mark.gpu
def test_gpu_step_reward_carries_the_repaired_minimum(bb, step_pool):
    """One zero-action step of 4096 envs (4 env groups, graph replay) from the 1..20 mm pool.  An
    env with no force on the person (info[:, 0] == 0) and no wiped target has the reward
    -w_distance d - w_velocity |v + w x (q tool_tip)| exactly: evaluated in float64 on the GPU's
    post-step state, with d the fp64 oracle's bb_closest there, the step's reward must lie within
    2e-5 (the 1e-5 m distance threshold plus fp32 rounding of a sum of order 1); misses are counted
    as in the query test (<= 0.4 %, no more than the fp32 oracle's distance misses on the same
    states within Poisson noise), and no env that queued a pair may be one.  Teeth: by
    avr_bb_closest_query on the post-step state, at least 5 force-free envs queued a pair whose rerun
    lowered the minimum by > 1e-4 m (the fp32 oracle's step predicts 512, test_step_pool_prediction),
    and at least half of the envs are force-free.  The query's minimum reproduces the reward: with
    the float64 velocity term within 1e-6 of the two terms' magnitudes (8 fp32 roundings: the
    cross product, the sum, the norm, the two products and their sum), and bit for bit through
    fp32 bb_reward where the velocity term is zero.  Measured (MI355X): 3215 of 4096 envs force-free, 0 reward misses (fp32 oracle 0), largest error
    2.4e-7; 48 force-free envs queued a pair, 33 with a repair > 1e-4 m (up to 4.8e-2 m), largest
    error on the queued 8.4e-8; reward against the query's minimum 1.8e-7 at most, 0.15 of the bound;
    no env with a zero velocity term."""
    from avr import _lib
    A, md = bb
    n = len(step_pool)
    S = step_pool.astype(np.float32)
    sim = _lib.Sim(md, n)
    try:
        assert sim.env_groups() == 4
        sim.set_state(S)
        ob, rew, done, info = sim.step(np.zeros((n, 7), np.float32))
        G = sim.get_state()
        q = sim.bb_closest_query().astype(np.float64)
    finally:
        sim.close()
    G64 = G.astype(np.float64)
    L = U.closest_labels(md, G64)
    wipe = slice(BB.S_TASK + BB.T_WIPE, BB.S_TASK + BB.T_WIPE + 6)
    free = (info[:, 0] == 0) & np.all(G[:, wipe] == S[:, wipe], axis=1)
    f = G64[:, BB.S_FREE:BB.S_FREE + 13]
    tip = _qrot(f[:, 3:7], np.array([md.desc.tool_tip[i] for i in range(3)]))
    vel = np.linalg.norm(f[:, 7:10] + np.cross(f[:, 10:13], tip), axis=1)
    wd, wv = float(md.desc.w_distance), float(md.desc.w_velocity)
    closed = -wd * L['d64'] - wv * vel
    err = np.abs(rew.astype(np.float64) - closed)
    miss = free & (err > 2e-5)
    n_g, n_32 = int(miss.sum()), int((free & (np.abs(L['d32'] - L['d64']) > MISS)).sum())
    queued = free & (q[:, 1] > 0)
    teeth = queued & (q[:, 2] - q[:, 0] > 1e-4)
    via_q = np.abs(rew.astype(np.float64) - (-wd * q[:, 0] - wv * vel))
    bound_q = 1e-6 * (np.abs(wd * q[:, 0]) + wv * (np.linalg.norm(f[:, 7:10], axis=1) + np.linalg.norm(np.cross(f[:, 10:13], tip), axis=1))) + 1e-9
    print('step: force-free %d of %d, reward misses %d (fp32 oracle distance misses %d), max err on force-free %.3g; queued force-free envs %d, '
          'max err on them %.3g; teeth %d (largest repair %.3g); reward vs the query\'s minimum: max %.3g, max / bound %.3g; zero-velocity envs %d'
          % (free.sum(), n, n_g, n_32, err[free].max(), queued.sum(), err[queued].max() if queued.any() else -1, teeth.sum(),
             float((q[:, 2] - q[:, 0])[queued].max()) if queued.any() else -1, via_q[free].max(), (via_q / bound_q)[free].max(), int((free & (vel == 0)).sum())))
    assert np.all(np.isfinite(rew)) and np.all(np.isfinite(q))
    assert free.mean() >= 0.5
    assert teeth.sum() >= 5
    assert n_g <= 0.004 * free.sum() and _poisson_ok(n_g, n_32), (n_g, n_32)
    assert not (queued & miss).any()
    assert np.all(via_q[free] <= bound_q[free])
    still = free & (vel == 0)
    if still.any():       # fp32 bb_reward with every other term zero
        r32 = np.float32(wd) * (-q[still, 0].astype(np.float32))
        assert np.array_equal(rew[still].view(np.uint32), r32.view(np.uint32))


@pytest.mark.gpu
def test_gpu_query_has_no_side_effects(bb, sim_q, pool):
    """The query leaves the state alone, and a step taken after queries (full and reduced capacity)
    equals bit for bit the same step on a handle that was never queried; the other tasks' handles
    refuse the hook with an error string."""
    from avr import _lib
    A, md = bb
    P, L = pool
    S = _padded(P)
    zero = np.zeros((E, 7), np.float32)
    sim_q.set_state(S)
    sim_q.bb_closest_query()
    sim_q.bb_closest_query(1)
    G = sim_q.get_state()
    assert np.array_equal(G.view(np.uint32), S.view(np.uint32))
    a = sim_q.step(zero) + (sim_q.get_state(),)
    ref = _lib.Sim(md, E)
    try:
        ref.set_state(S)
        b = ref.step(zero) + (ref.get_state(),)
    finally:
        ref.close()
    for x, y, name in zip(a, b, ('obs', 'rew', 'done', 'info', 'state')):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    Af = ABI.load_scene()
    other = _lib.Sim(ABI.ModelDesc(Af), 1)
    try:
        with pytest.raises(RuntimeError, match='avr_bb_closest_query'):
            other.bb_closest_query()
    finally:
        other.close()
