"""Part B's LDS-path sweeps (B4_ADDR): active-list entries that carry their addresses and clamped
row indices, so that an invalid step addresses a null row by construction.  The global-row path
(AVR_B4_GLOBAL=1) keeps its validity selects and out-of-bounds null addressing; both resolve the
same rows in the same order with the same arithmetic, so they agree bit for bit in states, outputs
and flags.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ('AVR_B4_GLOBAL', 'AVR_ENV_GROUPS', 'AVR_GRAPH')
LDS, GLB = '0', '1'
EMPTIED = (0, 9, 18)                    # envs without the bowl and the food: no contact, no friction unit


@pytest.fixture(scope='module')
def lib_and_scene(scene):
    from avr import _lib
    _lib.load()
    return scene


def make_sim(md, n, path, groups=1):
    """A handle created with AVR_B4_GLOBAL = path (and AVR_ENV_GROUPS) set; the environment is put back."""
    from avr import _lib
    old = {k: os.environ.pop(k, None) for k in KEYS}
    os.environ['AVR_B4_GLOBAL'] = path
    os.environ['AVR_ENV_GROUPS'] = str(groups)
    try:
        sim = _lib.Sim(md, n)
    finally:
        for k in KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    return sim


def reset_states(A, md, ids, impairment='none'):
    from avr import reset as RS
    S, _ = RS.batch_reset_states_fast(A, md, 1001, list(ids), impairment=impairment)
    return S.astype(np.float32)


def bits(x):
    """Bit patterns: equality that also holds a NaN to its payload and tells -0 from +0."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_outs(o1, o2):
    return len(o1) == len(o2) and all(len(a) == len(b) and all(same(x, y) for x, y in zip(a, b)) for a, b in zip(o1, o2))


@pytest.fixture(scope='module')
def mixed_states(lib_and_scene):
    """37 envs in one group: part-B block b holds envs x + 8 g + 32 j (x = b % 8, j = b / 8), so the
    blocks j = 1 hold one live env and three beyond n_envs.  'random' states for ids 0-26, 'tremor'
    for 27-36; envs 0, 9 and 18 have the bowl and the food far from the scene (no contact at all)
    and share their blocks with contact-rich envs."""
    from avr import _abi as ABI
    A, md = lib_and_scene
    S = np.concatenate([reset_states(A, md, range(0, 27), 'random'), reset_states(A, md, range(27, 37), 'tremor')])
    d = md.desc
    for f in [d.bowl_free] + list(range(d.food_free0, d.food_free0 + d.n_food)):
        o = ABI.S_FREE + ABI.FB_WORDS * f
        for e in EMPTIED:
            S[e, o:o + 3] = (50.0 + 2.0 * f, 50.0, 1.0)
    return S


def _run(md, S, path):
    """settle(20), 3 host-action steps, 3 device-random steps: (state, outputs, flags)."""
    import torch
    from avr import _abi as ABI, _lib
    n = len(S)
    sim = make_sim(md, n, path)
    assert sim.env_groups() == 1
    sim.set_state(S)
    outs = [(sim.settle(20),)]
    outs += [sim.step(_lib.random_actions(1001, np.arange(n), k)) for k in range(3)]
    dev = torch.device('cuda', 0)
    obs = torch.zeros(n, sim.obs_dim, device=dev)
    rew = torch.zeros(n, device=dev)
    done = torch.zeros(n, dtype=torch.uint8, device=dev)
    info = torch.zeros(n, ABI.INFO_DIM, device=dev)
    for k in range(3):
        sim.step_random_device(100 + k, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), info.data_ptr())
        sim.sync()
        outs.append(tuple(x.cpu().numpy() for x in (obs, rew, done, info)))
    G, flags = sim.get_state(), sim.get_flags()
    sim.close()
    return G, outs, flags


@pytest.fixture(scope='module')
def mixed_global(lib_and_scene, mixed_states):
    """The reference: the same library's global-row path, run once."""
    A, md = lib_and_scene
    return _run(md, mixed_states, GLB)


def test_mixed_block_agrees_bit_for_bit(lib_and_scene, mixed_states, mixed_global):
    from avr import _abi as ABI, _lib
    A, md = lib_and_scene
    G0, o0, f0 = mixed_global
    G, o, f = _run(md, mixed_states, LDS)
    ncp = G[:, ABI.S_TASK + ABI.T_NCP]
    print('T_NCP per env:', ncp.astype(int).tolist())
    # not vacuous: contact-rich envs, the emptied envs without any, unequal counts inside one block
    assert np.count_nonzero(ncp > 0) >= 20
    assert np.all(ncp[list(EMPTIED)] == 0)
    assert any(len(set(ncp[x:32:8].tolist())) > 1 for x in range(8))
    assert not np.any(f0 & _lib.FLAGS_FAULT_MASK)
    assert np.array_equal(f, f0)
    assert same(G, G0)
    assert len(o) == len(o0) == 7
    assert same_outs(o, o0)


def _masked(md, S, path):
    """Three steps, then a masked reset with two settle frames: every other env of blocks 0 and 1
    (envs 0, 8, 16, 24 and 1, 9, 17, 25) is masked off and runs null rows only."""
    from avr import _lib
    n = len(S)
    sim = make_sim(md, n, path)
    sim.set_state(S)
    for k in range(3):
        sim.step(_lib.random_actions(1001, np.arange(n), k))
    before = sim.get_state()
    mask = np.ones(n, np.uint8)
    mask[[8, 24, 1, 17]] = 0
    obs = np.full((n, sim.obs_dim), -7.0, np.float32)
    sim.reset(mask, S, 2, obs)
    after, flags = sim.get_state(), sim.get_flags()
    sim.close()
    return mask, before, after, obs, flags


def test_masked_envs_agree(lib_and_scene, mixed_states):
    A, md = lib_and_scene
    mask, b0, a0, obs0, f0 = _masked(md, mixed_states, GLB)
    _, b1, a1, obs1, f1 = _masked(md, mixed_states, LDS)
    keep = mask == 0
    assert same(a1[keep], b1[keep])                     # the masked-off envs were left alone
    assert np.all(obs1[keep] == -7.0) and np.all(obs1[~keep] != -7.0)
    assert same(b1, b0) and same(a1, a0) and same(obs1, obs0) and np.array_equal(f1, f0)


def _substep(md, S, path):
    sim = make_sim(md, len(S), path)
    sim.set_state(S)
    sim.substep(0.01)
    G, F = sim.get_state(), sim.get_flags()
    sim.close()
    return G, F


def test_one_substep_agrees(lib_and_scene):
    A, md = lib_and_scene
    S = np.concatenate([reset_states(A, md, range(0, 5), 'random'), reset_states(A, md, range(20, 23), 'tremor')])
    G0, F0 = _substep(md, S, GLB)
    G, F = _substep(md, S, LDS)
    assert same(G, G0) and np.array_equal(F, F0)


def _pr2_states(task, n):
    """n reset states of a PR2 task (the base-pose search runs on the device, as in bench.py), and,
    because a reset state has the tool clear of the person (no contact row at all), the same states
    with the tool pressed 2 mm into the arm, as the tasks' own GPU tests make them."""
    from avr import _abi as ABI, _lib
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
    return md, np.concatenate([S, C]).astype(np.float32)


@pytest.mark.parametrize('task', ['scratch', 'bedbath'])
def test_pr2_tasks_agree(lib_and_scene, task):
    """ScratchItchPR2 and BedBathingPR2: every row from LDS (non-contact rows included) against the
    global-row path, 8 envs from the reset path and their pressed-tool copies, 3 gym steps."""
    from avr import _abi as ABI, _lib
    t = ABI.TASK_SCRATCH if task == 'scratch' else ABI.TASK_BEDBATH
    md, S = _pr2_states(t, 8)
    n = len(S)
    assert n > 8                                        # the 8 reset states and at least one with contact
    L = ABI.SI if task == 'scratch' else ABI.BB
    res = []
    for path in (GLB, LDS):
        sim = make_sim(md, n, path)
        sim.set_state(S)
        outs, ncp = [], 0
        for k in range(3):
            outs.append(sim.step(_lib.random_actions(1001, np.arange(n), k) * 0.5))
            ncp += int(np.count_nonzero(sim.get_state()[:, L.S_TASK + L.T_NCP]))
        res.append((sim.get_state(), outs, sim.get_flags(), ncp))
        sim.close()
    (G0, o0, f0, ncp0), (G, o, f, ncp) = res
    print('contact env-steps', task, ncp0, 'of', 3 * n)
    assert ncp0 > 0 and ncp == ncp0
    assert same(G, G0) and np.array_equal(f, f0)
    assert same_outs(o, o0)


@pytest.mark.parametrize('task', ['feeding', 'scratch', 'bedbath'])
def test_part_b_resources(lib_and_scene, task):
    """Part B keeps its 40960 B of LDS (four blocks per CU) and uses no scratch, on every task."""
    from avr import _abi as ABI
    if task == 'feeding':
        A, md = lib_and_scene
    else:
        md = ABI.ModelDesc(ABI.load_scene(ABI.TASK_SCRATCH if task == 'scratch' else ABI.TASK_BEDBATH))
    sim = make_sim(md, 4, LDS)
    ki = sim.kernel_info()
    sim.close()
    assert ki['b']['scratch_bytes'] == 0
    assert ki['b']['lds_bytes'] == 40960
