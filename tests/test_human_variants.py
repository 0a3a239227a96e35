"""Human height variants inside one handle (include/avr.h avr_human_variants_set).

The reference's *New-v0 ids draw a new hipbone_to_mouth_height at every reset (feeding.py:170-172)
and rebuild the human.  Here a handle holds up to 64 height variants; an env picks one through the
T_GENDER word of its state row (0 / 1: the handle's base male / female, 2 + v: variant v).  A
variant carries the fp32 records that differ from the base scene for its gender, computed by the
model compiler from the scene rebuilt at {gender: height} and rounded as avr_create rounds a whole
scene -- so an env at variant (g, h) of a mixed handle must be bit-identical to the same env in a
handle created from scene_arrays(name, {g: h}).
"""
import functools

import numpy as np
import pytest

from avr import _abi as ABI
from avr import model_compiler as MC

TASKS = [ABI.TASK_FEEDING, ABI.TASK_SCRATCH, ABI.TASK_BEDBATH]
# the mixed handle of the GPU tests: env e uses variant e % 6
VARIANTS = [('male', 0.50), ('male', 0.60), ('male', 0.70), ('female', 0.44), ('female', 0.54), ('female', 0.64)]
N_ENVS = 8


# --------------------------------------------------------------------------------------- CPU
def _f32_tables(A):
    return {k: np.asarray(A[k], np.float32) for k in MC.VARIANT_DEVICE_ARRAYS if k in A}


@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('gender,height', [('male', 0.50), ('male', 0.70), ('female', 0.44), ('female', 0.64)])
def test_variant_records_rebuild_the_single_height_scene(task, gender, height):
    """The base scene's fp32 tables with the variant's records substituted are, bit for bit, the
    fp32 tables of scene_arrays(name, {g: h}) -- for every array a height changes -- and no other
    array of the scene differs."""
    name = ABI.SCENES[task]
    base = MC.scene_arrays(name)
    want = MC.scene_arrays(name, {gender: height})
    R = MC.human_variant_records(name, gender, height)
    got = MC.apply_variant_records(_f32_tables(base), R)
    changed = 0
    for k, w in _f32_tables(want).items():
        assert got[k].dtype == np.float32 and got[k].tobytes() == w.tobytes(), k
        changed += int(not np.array_equal(np.asarray(base[k], np.float32), w))
    assert changed >= 5                                   # (the records are not vacuous)
    np.testing.assert_array_equal(R['human_pos'], want['human_%s_pos' % gender])
    known = set(MC.VARIANT_DEVICE_ARRAYS) | set(MC.VARIANT_HOST_ARRAYS) | {'human_heights'}
    for k in want:
        if k not in known:
            assert np.array_equal(base[k], want[k]), 'a height changes %s, which no variant record carries' % k
    # the records touch this gender's rows only
    other = 1 - R['gender']
    assert not np.any(base['shape_gender'][R['shapes']] == other)
    assert np.all(base['body_kind'][R['bodies']] == ABI.BODY_HUMAN)
    assert R['gender'] == MC.GENDERS.index(gender) and R['height'] == height


def test_variant_argument_errors():
    with pytest.raises(ValueError):
        MC.human_variant_records('feeding_jaco', 'male', 0.29)        # MC.human_heights' [0.3, 1.0]
    with pytest.raises(ValueError):
        MC.human_variant_records('feeding_jaco', 'female', 1.01)
    with pytest.raises(ValueError):
        MC.human_variant_records('feeding_jaco', 'child', 0.5)
    from avr import env as EV
    with pytest.raises(ValueError):
        EV.variant_table({'male': list(np.linspace(0.5, 0.7, 65))})   # 65 variants > 64
    with pytest.raises(ValueError):
        EV.variant_table({'male': [0.6], 'child': [0.5]})
    with pytest.raises(ValueError):
        EV.variant_table({'male': [0.6, 1.2]})
    assert EV.variant_table({'male': 0.66}) is None                   # a scalar keeps its meaning: one rebuilt scene
    T = EV.variant_table({'male': [0.5, 0.7], 'female': [0.54]})
    assert T == [('male', 0.5), ('male', 0.7), ('female', 0.54)]


def test_variant_draw_is_uniform_reproducible_and_shard_independent():
    """The per-episode variant draw: uniform over the env's gender's list, a function of (seed,
    global env id, episode) alone -- two shards of 4 envs draw what one batch of 8 draws."""
    from avr import reset as RS
    ids = np.arange(8)
    a = RS.variant_draw(1001, ids, np.zeros(8, int), 21)
    b = np.concatenate([RS.variant_draw(1001, ids[:4], np.zeros(4, int), 21), RS.variant_draw(1001, ids[4:], np.zeros(4, int), 21)])
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, RS.variant_draw(1001, ids, np.zeros(8, int), 21))
    assert not np.array_equal(a, RS.variant_draw(1001, ids, np.ones(8, int), 21))       # a second episode redraws
    assert not np.array_equal(a, RS.variant_draw(1002, ids, np.zeros(8, int), 21))
    big = RS.variant_draw(7, np.arange(21000), np.zeros(21000, int), 21)
    assert big.min() == 0 and big.max() == 20
    cnt = np.bincount(big, minlength=21)
    assert np.abs(cnt - 1000).max() < 5 * np.sqrt(1000 * 20 / 21)                       # 5 sigma of a binomial count
    assert np.all(RS.variant_draw(1001, ids, np.zeros(8, int), 1) == 0)


def test_feeding_reset_states_unchanged_by_the_variant_stream():
    """FeedingJaco-v0's reset draws are untouched: the variant draw reads a counter index past the
    ones the reset uses, and a handle without variants never asks for it."""
    from avr import reset as RS
    A = ABI.load_scene(ABI.TASK_FEEDING)
    md = ABI.ModelDesc(A)
    S0, _ = RS.batch_reset_states_fast(A, md, 1001, list(range(4)), impairment='tremor', stream='philox')
    RS.variant_draw(1001, np.arange(4), np.zeros(4, int), 21)
    S1, _ = RS.batch_reset_states_fast(A, md, 1001, list(range(4)), impairment='tremor', stream='philox')
    np.testing.assert_array_equal(S0, S1)
    # the draw's counter index lies past every index the reset's own draws read (PH_INIT + restarts * n_arm)
    assert RS.PH_VARIANT >= RS.PH_INIT + 64 * len(md.arm_dofs)


def test_reset_inputs_pose_each_env_with_its_variant():
    """The host reset with variants: the slot goes to T_GENDER, the human is posed with the
    variant's link origins -- equal to the reset on the single-height scene -- and every other draw
    (gender, impairment, head angles, bowl, target, IK restarts) is the one without variants.  A
    variant at the default height reproduces the base reset but for the slot word."""
    from avr import reset as RS
    A = ABI.load_scene(ABI.TASK_FEEDING)
    md = ABI.ModelDesc(A)
    recs = [MC.human_variant_records('feeding_jaco', g, h) for g, h in VARIANTS]
    ctx = dict(slots={'male': [2, 3, 4], 'female': [5, 6, 7]}, pos={2 + v: R['human_pos'] for v, R in enumerate(recs)}, draw='uniform')
    ids = list(range(16))
    base = RS.reset_inputs(A, md, 1001, ids, impairment='tremor', stream='philox')
    var = RS.reset_inputs(A, md, 1001, ids, impairment='tremor', stream='philox', variants=ctx)
    for k in (1, 2):                                                   # target7, init
        np.testing.assert_array_equal(base[k], var[k])
    g_col = ABI.S_TASK + ABI.T_GENDER
    hs = slice(ABI.S_HUMAN, ABI.S_HUMAN + 7 * ABI.MAX_HUMAN)
    tg = slice(ABI.S_TASK + ABI.T_TARGET, ABI.S_TASK + ABI.T_TARGET + 3)
    slots = var[0][:, g_col].astype(int)
    assert len(set(slots)) >= 4 and slots.min() >= 2
    for e in ids:
        g, h = VARIANTS[slots[e] - 2]
        assert g == base[4][e]['gender'] == var[4][e]['gender'] and var[4][e]['slot'] == slots[e]
        A_h = recs[slots[e] - 2]['arrays']
        one = RS.reset_inputs(A_h, ABI.ModelDesc(A_h), 1001, [e], impairment='tremor', stream='philox')[0][0]
        np.testing.assert_array_equal(var[0][e, hs], one[hs])
        np.testing.assert_array_equal(var[0][e, tg], one[tg])
        rest = np.ones(ABI.STATE_WORDS, bool)
        rest[hs] = rest[tg] = rest[g_col] = False
        np.testing.assert_array_equal(var[0][e, rest], base[0][e, rest])
        if h == MC.DEFAULT_HEIGHT[g]:
            rest[hs] = rest[tg] = True
            np.testing.assert_array_equal(var[0][e, rest], base[0][e, rest])
    # shards draw what one batch draws; an explicit assignment overrides the draw
    two = np.concatenate([RS.reset_inputs(A, md, 1001, ids[:8], impairment='tremor', stream='philox', variants=ctx)[0],
                          RS.reset_inputs(A, md, 1001, ids[8:], impairment='tremor', stream='philox', variants=ctx)[0]])
    np.testing.assert_array_equal(two, var[0])
    pin = RS.reset_inputs(A, md, 1001, [0], genders=['female'], stream='philox', variants=dict(ctx, assign={0: 7}))[0]
    assert pin[0, g_col] == 7
    with pytest.raises(ValueError):
        RS.reset_inputs(A, md, 1001, [0], genders=['female'], stream='philox', variants=dict(ctx, assign={0: 2}))
    with pytest.raises(ValueError):
        RS.reset_inputs(A, md, 1001, [0], stream='numpy', variants=ctx)


# --------------------------------------------------------------------------------------- GPU
def _qrot(q, v):
    x, y, z, w = q
    u = np.array([x, y, z])
    return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


def _ids(v):
    return [e for e in range(N_ENVS) if e % len(VARIANTS) == v]


def _touch_human(A_h, L, row, gender):
    """Move a free body of the env (Feeding's first food item, the PR2's tool) onto the centre of a
    capsule of the env's human that its height moves, so that the variant's shape rows are in the
    narrowphase and the contact pool."""
    task = ABI.scene_task(A_h)
    g = MC.GENDERS.index(gender)
    base = ABI.load_scene(task)
    cand = np.nonzero((A_h['shape_gender'] == g) & (A_h['shape_kind'] == MC.CAPSULE))[0]
    moved = [s for s in cand if not np.array_equal(A_h['shape_pose'][s], base['shape_pose'][s])] or list(cand)
    s = moved[0]
    slot = int(A_h['body_index'][A_h['shape_body'][s]])
    hp = row[L.S_HUMAN + 7 * slot:L.S_HUMAN + 7 * slot + 7].astype(np.float64)
    c = hp[:3] + _qrot(hp[3:7], A_h['shape_pose'][s][:3])
    f = L.S_FREE + ABI.FB_WORDS * (2 if task == ABI.TASK_FEEDING else 0)
    row[f:f + 3] = c.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _setup(task):
    """Per task, computed once and shared read-only: the six variants' records and single-height
    model descriptors, and the host reset's state rows (env e at variant e % 6; FeedingJaco with
    impairment 'tremor', the PR2 tasks' arm chain is live in every reset state), with the gender in
    the T_GENDER word: S as reset, T with a free body moved onto the human."""
    name = ABI.SCENES[task]
    recs = [MC.human_variant_records(name, g, h) for g, h in VARIANTS]
    mds = [ABI.ModelDesc(R['arrays']) for R in recs]
    A0 = ABI.load_scene(task)
    md0 = ABI.ModelDesc(A0)
    L = md0.layout
    genders = [VARIANTS[e % len(VARIANTS)][0] for e in range(N_ENVS)]
    if task == ABI.TASK_FEEDING:
        # one reset call for the eight envs (the host IK dominates its cost), each posed with its variant
        from avr import reset as RS
        ctx = dict(slots={'male': [2, 3, 4], 'female': [5, 6, 7]}, pos={2 + v: R['human_pos'] for v, R in enumerate(recs)}, draw=None,
                   assign={e: 2 + e % len(VARIANTS) for e in range(N_ENVS)})
        S = np.asarray(RS.batch_reset_states_fast(A0, md0, 1001, list(range(N_ENVS)), genders=genders, impairment='tremor', stream='philox',
                                                  variants=ctx)[0], np.float32)
        dt = 0.01
    else:
        S = np.zeros((N_ENVS, L.STATE_WORDS), np.float32)
        for v, (g, h) in enumerate(VARIANTS):
            A_h = recs[v]['arrays']
            if task == ABI.TASK_SCRATCH:
                from avr import reset_scratch as RSS
                rows = RSS.batch_reset_states(A_h, mds[v], 1001, _ids(v), genders=[g] * len(_ids(v)), attempts=12, iters=80)[0]
            else:
                from avr import reset_bedbath as RBB
                rows = RBB.batch_reset_states(A_h, mds[v], 1001, _ids(v), genders=[g] * len(_ids(v)), attempts=12)[0]
            S[_ids(v)] = rows
        dt = 0.02
    S[:, L.S_TASK + L.T_GENDER] = [MC.GENDERS.index(g) for g in genders]
    T = S.copy()
    for e in range(N_ENVS):
        _touch_human(recs[e % len(VARIANTS)]['arrays'], L, T[e], genders[e])
    S.setflags(write=False)
    T.setflags(write=False)
    return dict(recs=recs, mds=mds, md0=md0, L=L, S=S, T=T, dt=dt)


def _with_slots(S, L):
    M = np.array(S)
    M[:, L.S_TASK + L.T_GENDER] = [2 + e % len(VARIANTS) for e in range(len(M))]
    return M


@pytest.fixture(scope='module')
def handles():
    """Eight-env handles shared by the tests of this module (creating a FeedingJaco handle takes a
    couple of seconds): get(task, 'mixed') holds the six variants, get(task, v) is the single-height
    handle of variant v, get(task, 'base') a default handle that never saw a variant call.  Every
    user uploads its own state first.  run(task, key) caches a handle's states after one sub-step
    and after 5 gym steps from the rows T."""
    from avr import _lib
    sims, runs = {}, {}

    def get(task, key):
        if (task, key) not in sims:
            U = _setup(task)
            sim = _lib.Sim(U['md0'] if key in ('mixed', 'base') else U['mds'][key], N_ENVS)
            if key == 'mixed':
                sim.human_variants_set(U['recs'])
            sims[task, key] = sim
        return sims[task, key]

    def run(task, key):
        if (task, key) not in runs:
            U = _setup(task)
            sim = get(task, key)
            S = _with_slots(U['T'], U['L']) if key == 'mixed' else np.array(U['T'])
            sim.set_state(S)
            sim.substep(U['dt'])
            one = sim.get_state()
            sim.set_state(S)
            for t in range(5):
                sim.step(_lib.random_actions(1001, np.arange(N_ENVS), t))
            runs[task, key] = (one, sim.get_state())
        return runs[task, key]

    get.run = run
    yield get
    for sim in sims.values():
        sim.close()


def _human_in_pool(md, L, row):
    n = int(row[L.S_TASK + L.T_NCP])
    cp = row[L.S_CP:L.S_CP + n * ABI.CP_WORDS].reshape(n, ABI.CP_WORDS)
    kinds = md.A['body_kind'][md.A['shape_body'][cp[:, [ABI.CP_SA, ABI.CP_SB]].astype(int)]]
    return n > 0 and bool(np.any(kinds == ABI.BODY_HUMAN))


@pytest.mark.gpu
@pytest.mark.parametrize('v', range(len(VARIANTS)))
@pytest.mark.parametrize('task', TASKS)
def test_mixed_handle_is_bit_identical_to_single_height_handle(task, v, handles):
    """One handle with six variants, env e at variant e % 6, against the single-height handle of
    variant v fed the same rows with the slot mapped back to the gender: after one sub-step and
    after 5 gym steps with random actions the variant's envs' state rows are equal, contact pool
    included.  At least one env of the task holds a contact with a human body after the sub-step
    (the scaled capsules are in play)."""
    U = _setup(task)
    L = U['L']
    g, h = VARIANTS[v]
    g_col = L.S_TASK + L.T_GENDER
    assert [(MC.GENDERS[gi], round(hi, 6)) for gi, hi in handles(task, 'mixed').human_variants()] == VARIANTS
    mixed, single = handles.run(task, 'mixed'), handles.run(task, v)
    assert sum(_human_in_pool(U['md0'], L, mixed[0][e]) for e in range(N_ENVS)) >= 1
    for got, want in zip(mixed, single):
        a, b = got[_ids(v)].copy(), want[_ids(v)].copy()
        assert np.all(a[:, g_col] == 2 + v) and np.all(b[:, g_col] == MC.GENDERS.index(g))
        a[:, g_col] = b[:, g_col]
        assert np.array_equal(a, b), (task, g, h, np.nonzero(a != b))
    if h != MC.DEFAULT_HEIGHT[g]:
        # the height matters: the same rows in the default handle come out differently
        base = handles(task, 'base')
        base.set_state(np.array(U['T']))
        base.substep(U['dt'])
        assert not np.array_equal(base.get_state()[_ids(v)], single[0][_ids(v)])


@pytest.mark.gpu
@pytest.mark.parametrize('task', TASKS)
def test_mixed_handle_substep_matches_per_height_oracles(task, handles):
    """The mixed handle, one sub-step from the plain reset rows, against the fp64 oracle on each
    height's scene: test_human_heights' tolerances (|dq| < 1e-5 rad, free bodies < 1e-4)."""
    from oracle.oracle import Oracle
    U = _setup(task)
    L, S = U['L'], U['S']
    sim = handles(task, 'mixed')
    sim.set_state(_with_slots(S, L))
    sim.substep(U['dt'])
    G = sim.get_state()
    fb = slice(L.S_FREE, L.S_FREE + L.MAX_FREE * ABI.FB_WORDS)
    for v, (g, h) in enumerate(VARIANTS):
        md_h = U['mds'][v]
        o = Oracle(md_h, len(_ids(v)))
        o.set_threads(8)
        o.set_state(np.array(S[_ids(v)], np.float64))
        o.substep(U['dt'])
        C = o.get_state()
        nd = min(md_h.n_dof + L.HC_N, L.MAX_DOF)
        assert np.abs(G[_ids(v), :nd] - C[:, :nd]).max() < 1e-5, (g, h)
        assert np.abs(G[_ids(v)][:, fb] - C[:, fb]).max() < 1e-4, (g, h)


@pytest.mark.gpu
@pytest.mark.parametrize('task', TASKS)
def test_no_variants_is_the_base_handle(task, handles):
    """avr_human_variants_set(sim, 0, NULL) on a default handle, and variants loaded and cleared
    again, leave 5 gym steps bit-identical to a handle that never called it."""
    from avr import _lib
    U = _setup(task)

    def five(sim):
        sim.set_state(np.array(U['S']))
        for t in range(5):
            sim.step(_lib.random_actions(1001, np.arange(N_ENVS), t))
        return sim.get_state()

    want = five(handles(task, 'base'))
    sim = _lib.Sim(U['md0'], N_ENVS)
    sim.human_variants_set([])
    assert sim.human_variants() == []
    empty = five(sim)
    sim.human_variants_set(U['recs'])
    sim.human_variants_set([])
    assert sim.human_variants() == []
    cleared = five(sim)
    sim.close()
    assert np.array_equal(want, empty) and np.array_equal(want, cleared)


@pytest.mark.gpu
def test_unloaded_slot_is_refused_everywhere():
    """A row whose slot is 2 + n_var is refused by set_state, set_state_masked, reset, reset_ik and
    reset_pool_set: a negative return code, avr_last_error names the call and the slot, and the
    device state is untouched (nothing was copied or launched)."""
    from avr import _lib
    U = _setup(ABI.TASK_FEEDING)
    L = U['L']
    n = 4
    sim = _lib.Sim(U['md0'], n)
    good = np.array(U['S'][:n])
    for n_var in (0, 3):
        sim.human_variants_set(U['recs'][:n_var])
        sim.set_state(good)
        before = sim.get_state()
        bad = good.copy()
        bad[2, L.S_TASK + L.T_GENDER] = 2 + n_var
        obs = np.zeros((n, sim.obs_dim), np.float32)
        mask = np.ones(n, np.uint8)
        t7 = np.zeros((n, 7), np.float32)
        init = np.zeros((n, 1, 7), np.float32)
        calls = {
            'avr_set_state': lambda: sim.lib.avr_set_state(sim.h, bad.ctypes.data),
            'avr_set_state_masked': lambda: sim.lib.avr_set_state_masked(sim.h, mask.ctypes.data, bad.ctypes.data),
            'avr_reset': lambda: sim.lib.avr_reset(sim.h, None, bad.ctypes.data, 2, obs.ctypes.data),
            'avr_reset_pool_set': lambda: sim.lib.avr_reset_pool_set(sim.h, n, bad.ctypes.data, obs.ctypes.data),
            'avr_reset_ik': lambda: sim.lib.avr_reset_ik(sim.h, None, bad.ctypes.data, t7.ctypes.data, init.ctypes.data, None, 1, 1, 0.01, None, 0,
                                                         obs.ctypes.data, None),
        }
        for name, call in calls.items():
            rc = call()
            msg = sim.lib.avr_last_error(sim.h).decode()
            assert rc < 0, name
            assert msg.startswith(name + ':') and 'slot %d' % (2 + n_var) in msg, (name, msg)
            assert np.array_equal(sim.get_state(), before), name
        for w in (-1.0, 0.5, np.nan):
            bad[2, L.S_TASK + L.T_GENDER] = w
            assert sim.lib.avr_set_state(sim.h, bad.ctypes.data) < 0
        # a masked-out bad row is not looked at; the loaded slots pass
        mask[2] = 0
        assert sim.lib.avr_set_state_masked(sim.h, mask.ctypes.data, bad.ctypes.data) == 0
        if n_var:
            okrow = good.copy()
            okrow[:, L.S_TASK + L.T_GENDER] = [2, 3, 4, 1]
            sim.set_state(okrow)
    with pytest.raises(RuntimeError):
        sim.human_variants_set([U['recs'][0]] * 65)
    short = dict(U['recs'][0], shapes=U['recs'][0]['shapes'][:-1])
    with pytest.raises(RuntimeError):
        sim.human_variants_set([short])                   # a record compiled for another scene
    sim.close()


@pytest.mark.gpu
def test_rollover_carries_the_pool_rows_slot(handles):
    """FeedingJaco, 4 envs, a pool of 8 settled rows with mixed slots: with T_ITER at max_steps - 1
    the first of two rollout steps rolls every env over; each env's slot and human slot poses are
    its pool row's, and its next step equals, bit for bit, the step of the single-height handle
    from that pool row."""
    import torch
    from avr import _lib
    task = ABI.TASK_FEEDING
    U = _setup(task)
    L = U['L']
    n, seed = 4, 1001
    pool = handles(task, 'mixed')
    obs = pool.reset(None, _with_slots(U['S'], L), frames=20)
    P = pool.get_state()
    sim = _lib.Sim(U['md0'], n, seed=seed)
    sim.human_variants_set(U['recs'])
    sim.reset_pool_set(P, obs)
    S = np.array(P[:n])
    S[:, L.S_TASK + L.T_ITER] = int(U['md0'].params['max_episode_steps']) - 1
    sim.set_state(S)
    sim.rollover_enable(True)
    d_obs = torch.zeros((n, sim.obs_dim), device='cuda')
    d_rew = torch.zeros(n, device='cuda')
    d_done = torch.zeros(n, dtype=torch.uint8, device='cuda')
    d_info = torch.zeros((n, ABI.INFO_DIM), device='cuda')
    sim.rollout_random_device(0, 1, d_obs.data_ptr(), d_rew.data_ptr(), d_done.data_ptr(), d_info.data_ptr())
    sim.sync()
    assert d_done.cpu().numpy().all()
    R = sim.get_state()
    rows = _lib.rollover_index(seed, np.arange(n), 0, len(P))
    hs = slice(L.S_HUMAN, L.S_HUMAN + 7 * L.MAX_HUMAN)
    for e in range(n):
        assert R[e, L.S_TASK + L.T_GENDER] == P[rows[e], L.S_TASK + L.T_GENDER] == 2 + rows[e] % len(VARIANTS)
        assert np.array_equal(R[e, hs], P[rows[e], hs])
        assert np.array_equal(R[e], P[rows[e]])
    sim.rollout_random_device(1, 1, d_obs.data_ptr(), d_rew.data_ptr(), d_done.data_ptr(), d_info.data_ptr())
    sim.sync()
    N = sim.get_state()
    sim.close()
    a1 = _lib.random_actions(seed, np.arange(N_ENVS), 1)
    for e in range(n):
        v = int(rows[e]) % len(VARIANTS)
        one = handles(task, v)
        row = P[rows[e]].copy()
        row[L.S_TASK + L.T_GENDER] = MC.GENDERS.index(VARIANTS[v][0])
        one.set_state(np.tile(row, (N_ENVS, 1)))
        one.step(a1)                    # (row e steps with env e's action of step 1, as the rollout drew it)
        want = one.get_state()[e]
        got = N[e].copy()
        got[L.S_TASK + L.T_GENDER] = want[L.S_TASK + L.T_GENDER]
        assert np.array_equal(got, want), e


