"""Switches that only change which lane or wave does a piece of work, off against on, bit for bit.

AVR_NP_HOT=0|1: the narrowphase's sphere-hull blocks start the shape pairs that hold a point in the
env's contact pool, and those that took long in the sub-step before, ahead of the others.  Results
are stored by pair index, so the order changes no bit of any state, output or flag.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = {'np_hot': 'AVR_NP_HOT'}
KEYS = tuple(SWITCHES.values()) + ('AVR_PAIRS_FLAT', 'AVR_DYN_SPLIT', 'AVR_ENV_GROUPS', 'AVR_B4_GLOBAL', 'AVR_GRAPH')
OFF, ON = 0, 1
MIN_POINTS = 8                  # contact points an env must hold for the reorder to act on it


@pytest.fixture(scope='module')
def lib_and_scene(scene):
    from avr import _lib
    _lib.load()
    return scene


def make_sim(md, n, switch, v, groups=None):
    """A handle created with the switch's variable = v (and AVR_ENV_GROUPS) set; the environment is put back."""
    from avr import _lib
    old = {k: os.environ.pop(k, None) for k in KEYS}
    os.environ[SWITCHES[switch]] = str(v)
    if groups:
        os.environ['AVR_ENV_GROUPS'] = str(groups)
    try:
        sim = _lib.Sim(md, n)
    finally:
        for k in KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    assert getattr(sim, switch)() == v
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
def settled(lib_and_scene):
    """100 FeedingJaco envs, 70 'random' and 30 'tremor' reset states (both DoF counts), and the same
    states after settle(20) (computed once, with every switch at its default)."""
    from avr import _lib
    A, md = lib_and_scene
    raw = np.concatenate([reset_states(A, md, range(0, 70), 'random'), reset_states(A, md, range(70, 100), 'tremor')])
    sim = _lib.Sim(md, len(raw))
    sim.set_state(raw)
    sim.settle(20)
    S = sim.get_state()
    sim.close()
    return raw, S


def _ncp(G):
    from avr import _abi as ABI
    return G[:, ABI.S_TASK + ABI.T_NCP]


def _steps(md, S, switch, v, fresh=None):
    """Three gym steps in groups of 32 / 32 / 36; with `fresh` = (mask, raw states), the masked envs
    are put back to their raw reset states (an empty contact pool) after the first step.  Returns
    (states after each step, outputs, flags, contact counts at the start of each step)."""
    from avr import _lib
    n = len(S)
    sim = make_sim(md, n, switch, v, groups=3)
    assert sim.env_groups() == 3
    sim.set_state(S)
    states, outs, ncp0 = [], [], []
    for k in range(3):
        if fresh is not None and k == 1:
            sim.set_state_masked(fresh[0], fresh[1])
        ncp0.append(_ncp(sim.get_state()).copy())
        outs.append(sim.step(_lib.random_actions(1001, np.arange(n), k)))
        states.append(sim.get_state())
    flags = sim.get_flags()
    sim.close()
    return states, outs, flags, ncp0


@pytest.mark.parametrize('switch', sorted(SWITCHES))
def test_plain_run_agrees(lib_and_scene, settled, switch):
    from avr import _lib
    A, md = lib_and_scene
    _, S = settled
    G0, o0, f0, n0 = _steps(md, S, switch, OFF)
    G1, o1, f1, n1 = _steps(md, S, switch, ON)
    for c in n0:                            # the reorder acts: pools are full where the compared sub-steps start
        print('envs with %d or more points: %d of %d, mean %.1f' % (MIN_POINTS, np.count_nonzero(c >= MIN_POINTS), len(c), c.mean()))
        assert np.count_nonzero(c >= MIN_POINTS) >= 0.9 * len(c)
    assert not np.any(f0 & _lib.FLAGS_FAULT_MASK)
    assert np.array_equal(f0, f1)
    assert all(same(a, b) for a, b in zip(G0, G1))
    assert same_outs(o0, o1)


@pytest.mark.parametrize('switch', sorted(SWITCHES))
def test_masked_reset_in_the_middle_agrees(lib_and_scene, settled, switch):
    """Every third env goes back to its raw reset state (no contact point yet) after the first step:
    empty pools beside full ones in the same launches."""
    A, md = lib_and_scene
    raw, S = settled
    mask = np.zeros(len(S), np.uint8); mask[::3] = 1
    assert np.all(_ncp(raw) == 0)
    G0, o0, f0, n0 = _steps(md, S, switch, OFF, fresh=(mask, raw))
    G1, o1, f1, n1 = _steps(md, S, switch, ON, fresh=(mask, raw))
    assert np.all(n0[1][mask == 1] == 0)
    assert np.count_nonzero(n0[1][mask == 0] >= MIN_POINTS) >= 0.9 * np.count_nonzero(mask == 0)
    assert np.count_nonzero(n0[2] >= MIN_POINTS) >= 0.9 * len(S)          # the reset envs' pools have filled again
    assert np.array_equal(f0, f1)
    assert all(same(a, b) for a, b in zip(G0, G1))
    assert same_outs(o0, o1)


def _substeps(md, S, switch, v, k):
    sim = make_sim(md, len(S), switch, v)
    sim.set_state(S)
    G = []
    for _ in range(k):
        sim.substep(0.01)
        G.append(sim.get_state())
    F = sim.get_flags()
    sim.close()
    return G, F


@pytest.mark.parametrize('switch', sorted(SWITCHES))
def test_truncated_list_agrees(lib_and_scene, switch):
    """Every free body (spoon, bowl, food) at the bowl's position: the shape-pair list overflows its
    MAXSP entries (flag bit 3).  Two sub-steps: the second starts from the pool the first left."""
    from avr import _abi as ABI
    A, md = lib_and_scene
    S = reset_states(A, md, range(2))
    bowl = ABI.S_FREE + ABI.FB_WORDS * md.desc.bowl_free
    for f in range(ABI.MAX_FREE):
        S[:, ABI.S_FREE + ABI.FB_WORDS * f:ABI.S_FREE + ABI.FB_WORDS * f + 3] = S[:, bowl:bowl + 3]
    G0, F0 = _substeps(md, S, switch, OFF, 2)
    G, F = _substeps(md, S, switch, ON, 2)
    print('T_NCP after the first sub-step:', _ncp(G0[0]).astype(int).tolist())
    assert np.all(_ncp(G0[0]) >= MIN_POINTS)            # the second sub-step starts from full pools
    assert np.all(F0 & 8) and np.array_equal(F, F0)     # truncated: the case is not empty
    assert all(same(a, b) for a, b in zip(G, G0))


def _pr2_states(task, n):
    """n reset states of a PR2 task and the same states with the tool pressed 2 mm into the arm (a reset
    state has the tool clear of the person: no contact row at all)."""
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
    return A, md, S.astype(np.float32), C.astype(np.float32)


@pytest.fixture(scope='module', params=['scratch', 'bedbath'])
def pr2(request, lib_and_scene):
    from avr import _abi as ABI
    task = request.param
    A, md, S, C = _pr2_states(ABI.TASK_SCRATCH if task == 'scratch' else ABI.TASK_BEDBATH, 8)
    assert len(C) > 0
    return task, md, S, C


@pytest.mark.parametrize('switch', sorted(SWITCHES))
def test_pr2_tasks_agree(pr2, switch):
    """ScratchItchPR2 and BedBathingPR2: 8 envs from the reset path and their pressed-tool copies, 3 gym steps."""
    from avr import _abi as ABI, _lib
    task, md, S0, C = pr2
    S = np.concatenate([S0, C])
    n = len(S)
    L = ABI.SI if task == 'scratch' else ABI.BB
    res = []
    for v in (OFF, ON):
        sim = make_sim(md, n, switch, v)
        sim.set_state(S)
        outs, states = [], []
        for k in range(3):
            outs.append(sim.step(_lib.random_actions(1001, np.arange(n), k) * 0.5))
            states.append(sim.get_state())
        res.append((states, outs, sim.get_flags()))
        sim.close()
    (G0, o0, f0), (G, o, f) = res
    ncp = np.stack([g[len(S0):, L.S_TASK + L.T_NCP] for g in G0])
    print('contact points of the pressed envs after each step', task, ncp.astype(int).tolist())
    assert ncp.max() > 0                                # contacts were exercised
    assert np.array_equal(f, f0)
    assert all(same(a, b) for a, b in zip(G, G0))
    assert same_outs(o, o0)


@pytest.mark.parametrize('switch', sorted(SWITCHES))
@pytest.mark.parametrize('v', [OFF, ON])
def test_resources_and_report(lib_and_scene, switch, v):
    A, md = lib_and_scene
    sim = make_sim(md, 4, switch, v)                    # (checks that the report function returns what was set)
    ki = sim.kernel_info()
    sim.close()
    assert all(k['scratch_bytes'] == 0 for k in ki.values())
    assert ki['narrowphase']['lds_bytes'] <= 4 * 1024   # staged entries, body frames, pool keys: 16 blocks per CU
    assert ki['narrowphase']['vgprs'] <= 128            # four waves per SIMD
