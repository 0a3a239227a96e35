"""The pair kernel's child-pair enumeration (AVR_PAIRS_FLAT=0|1): flat passes over all active body
pairs instead of one compound pair at a time.  The pair list is the same set in the same order,
so the switch changes no bit of any state, output or flag.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ('AVR_PAIRS_FLAT', 'AVR_DYN_SPLIT', 'AVR_ENV_GROUPS', 'AVR_B4_GLOBAL', 'AVR_GRAPH')
OFF, ON = 0, 1


@pytest.fixture(scope='module')
def lib_and_scene(scene):
    from avr import _lib
    _lib.load()
    return scene


def make_sim(md, n, cfg, groups=None):
    """A handle created with AVR_PAIRS_FLAT = cfg (and AVR_ENV_GROUPS) set; the environment is put back."""
    flat = cfg
    from avr import _lib
    old = {k: os.environ.pop(k, None) for k in KEYS}
    os.environ['AVR_PAIRS_FLAT'] = str(flat)
    if groups:
        os.environ['AVR_ENV_GROUPS'] = str(groups)
    try:
        sim = _lib.Sim(md, n)
    finally:
        for k in KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    assert sim.pairs_flat() == flat
    return sim


def reset_states(A, md, ids, impairment='none'):
    from avr import reset as RS
    S, _ = RS.batch_reset_states_fast(A, md, 1001, list(ids), impairment=impairment)
    return S.astype(np.float32)


def bits(x):
    """Bit patterns: equality that also holds a NaN to its payload."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _run(md, S, cfg):
    """settle(20), 3 host-action steps, 3 device-random steps: (state, outputs, flags)."""
    import torch
    from avr import _abi as ABI, _lib
    n = len(S)
    sim = make_sim(md, n, cfg, groups=3)
    assert sim.env_groups() == 3
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
def main_runs(lib_and_scene):
    """100 envs in groups of 32 / 32 / 36 (a partly filled run of role blocks), 70 'random' and 30
    'tremor' reset states (both DoF counts, both genders), once per configuration."""
    A, md = lib_and_scene
    S = np.concatenate([reset_states(A, md, range(0, 70), 'random'), reset_states(A, md, range(70, 100), 'tremor')])
    done = {}

    def get(cfg):                       # (each configuration runs once, in the first test that asks for it)
        if cfg not in done:
            done[cfg] = _run(md, S, cfg)
        return done[cfg]
    return get


def test_switch_agrees_bit_for_bit(main_runs, cfg=ON):
    from avr import _abi as ABI, _lib
    G1, o1, f1 = main_runs(OFF)
    Gw, ow, fw = main_runs(cfg)
    assert G1[:, ABI.S_TASK + ABI.T_NCP].max() > 0          # contacts (and so narrowphase hits) were exercised
    assert not np.any(f1 & _lib.FLAGS_FAULT_MASK)
    assert np.array_equal(f1, fw)
    assert np.array_equal(G1, Gw)
    assert len(o1) == len(ow) == 7
    for a, b in zip(o1, ow):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def _substep(md, S, cfg):
    sim = make_sim(md, len(S), cfg)
    sim.set_state(S)
    sim.substep(0.01)
    G, F = sim.get_state(), sim.get_flags()
    sim.close()
    return G, F


@pytest.fixture(scope='module')
def substep_off(lib_and_scene):
    A, md = lib_and_scene
    S = np.concatenate([reset_states(A, md, range(0, 5), 'random'), reset_states(A, md, range(20, 23), 'tremor')])
    return S, _substep(md, S, OFF)


def test_one_substep_agrees(lib_and_scene, substep_off, cfg=ON):
    A, md = lib_and_scene
    S, (G0, F0) = substep_off
    G, F = _substep(md, S, cfg)
    assert np.array_equal(G, G0) and np.array_equal(F, F0)


@pytest.fixture(scope='module')
def truncated_off(lib_and_scene):
    """Every free body (spoon, bowl, food) at the bowl's position: the shape-pair list overflows its
    MAXSP entries (flag bit 3): the flat enumeration's truncation at MAXSP, with compound pairs
    (food against the bowl's and the spoon's pieces) whose children all survive the cull."""
    from avr import _abi as ABI
    A, md = lib_and_scene
    S = reset_states(A, md, range(2))
    bowl = ABI.S_FREE + ABI.FB_WORDS * md.desc.bowl_free
    for f in range(ABI.MAX_FREE):
        S[:, ABI.S_FREE + ABI.FB_WORDS * f:ABI.S_FREE + ABI.FB_WORDS * f + 3] = S[:, bowl:bowl + 3]
    return S, _substep(md, S, OFF)


def test_truncated_list_agrees(lib_and_scene, truncated_off, cfg=ON):
    A, md = lib_and_scene
    S, (G0, F0) = truncated_off
    G, F = _substep(md, S, cfg)
    assert np.all(F0 & 8) and np.all(F & 8)             # both paths truncated the list: the case is not empty
    assert np.array_equal(F, F0)
    assert same(G, G0)


def test_mask_holds_with_the_switch_on(lib_and_scene, w=ON):
    from avr import _lib
    A, md = lib_and_scene
    n = 24
    S = reset_states(A, md, range(n))
    sim = make_sim(md, n, w)
    sim.set_state(S)
    for k in range(3):
        sim.step(_lib.random_actions(1001, np.arange(n), k))
    before = sim.get_state()
    mask = np.zeros(n, np.uint8); mask[::3] = 1
    obs = np.full((n, sim.obs_dim), -7.0, np.float32)
    sim.reset(mask, S, 2, obs)            # masked upload, then 2 masked settle frames (both roles' blocks)
    after = sim.get_state()
    keep = mask == 0
    assert np.array_equal(after[keep], before[keep])
    assert np.all(obs[keep] == -7.0) and np.all(obs[~keep] != -7.0)
    # the reset envs equal a fresh settle(2) of the same states
    ref = make_sim(md, n, w)
    ref.set_state(S)
    ref.settle(2)
    assert np.array_equal(after[~keep], ref.get_state()[~keep])
    sim.close(); ref.close()


def _pr2_states(task, n):
    """n reset states of a PR2 task (the base-pose search runs on the device, as in bench.py)."""
    from avr import _abi as ABI, _lib
    A = ABI.load_scene(task)
    md = ABI.ModelDesc(A)
    sim = _lib.Sim(md, 1)
    try:
        if task == ABI.TASK_BEDBATH:
            from avr import reset_bedbath as RBB
            S, _ = RBB.batch_reset_states(A, md, 1001, list(range(n)), sim=sim, device=0)
        else:
            from avr import reset_scratch as RSS
            S, _ = RSS.batch_reset_states(A, md, 1001, list(range(n)), sim=sim)
    finally:
        sim.close()
    return md, S.astype(np.float32)


@pytest.mark.parametrize('task', ['scratch', 'bedbath'])
def test_pr2_tasks_agree(lib_and_scene, task):
    """ScratchItchPR2 and BedBathingPR2 (the same kernel source): 32 envs, 2 gym steps."""
    from avr import _abi as ABI, _lib
    n = 32
    md, S = _pr2_states(ABI.TASK_SCRATCH if task == 'scratch' else ABI.TASK_BEDBATH, n)
    res = []
    for s in (OFF, ON):
        sim = make_sim(md, n, s)
        sim.set_state(S)
        outs = [sim.step(_lib.random_actions(1001, np.arange(n), k)) for k in range(2)]
        res.append((sim.get_state(), outs, sim.get_flags()))
        sim.close()
    G1, o1, f1 = res[0]
    for G, o, f in res[1:]:
        assert np.array_equal(G, G1) and np.array_equal(f, f1)
        for a, b in zip(o, o1):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)


@pytest.mark.parametrize('w', [OFF, ON])
def test_resources_and_report(lib_and_scene, w):
    A, md = lib_and_scene
    sim = make_sim(md, 4, w)                              # (checks that the report function returns what was set)
    ki = sim.kernel_info()
    assert set(ki) == {'pairs', 'narrowphase', 'a', 'b', 'task'}
    assert all(k['scratch_bytes'] == 0 for k in ki.values())
    assert ki['pairs']['lds_bytes'] <= 10240              # 16 blocks per CU
    assert ki['narrowphase']['lds_bytes'] <= 4 * 1024     # staged entries + body frames: 16 blocks per CU
    assert ki['narrowphase']['vgprs'] <= 128              # four waves per SIMD
    sim.close()
