"""The pair launch's dynamics role (AVR_DYN_SPLIT, FeedingJaco's default): the unconstrained
velocities and the non-contact rows run beside the pair enumeration instead of inside kernel a.
The moved code is the same device functions on the same inputs, so switching it changes no bit.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ('AVR_DYN_SPLIT', 'AVR_ENV_GROUPS', 'AVR_B4_GLOBAL', 'AVR_GRAPH')


@pytest.fixture(scope='module')
def lib_and_scene(scene):
    from avr import _lib
    _lib.load()
    return scene


def make_sim(md, n, split, groups=None):
    """A handle created with AVR_DYN_SPLIT (and AVR_ENV_GROUPS) set; the environment is put back."""
    from avr import _lib
    old = {k: os.environ.pop(k, None) for k in KEYS}
    os.environ['AVR_DYN_SPLIT'] = '1' if split else '0'
    if groups:
        os.environ['AVR_ENV_GROUPS'] = str(groups)
    try:
        return _lib.Sim(md, n)
    finally:
        for k in KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def reset_states(A, md, ids, impairment='none'):
    from avr import reset as RS
    S, _ = RS.batch_reset_states_fast(A, md, 1001, list(ids), impairment=impairment)
    return S.astype(np.float32)


def _run(md, S, split):
    """settle(20), 3 host-action steps, 3 device-random steps: (dyn_split, state, outputs, flags)."""
    import torch
    from avr import _abi as ABI, _lib
    n = len(S)
    sim = make_sim(md, n, split, groups=3)
    assert sim.env_groups() == 3
    on = sim.dyn_split()
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
    return on, G, outs, flags


def test_switch_on_and_off_agree_bit_for_bit(lib_and_scene):
    """100 envs in groups of 32 / 32 / 36 (a partly filled run of role blocks), both DoF counts
    (the tremor envs' head chain), food in the spoon and bowl (contact and robot-contact rows)."""
    from avr import _abi as ABI, _lib
    A, md = lib_and_scene
    S = np.concatenate([reset_states(A, md, range(0, 70), 'random'), reset_states(A, md, range(70, 100), 'tremor')])
    on1, G1, o1, f1 = _run(md, S, True)
    on0, G0, o0, f0 = _run(md, S, False)
    assert (on1, on0) == (1, 0)
    assert G1[:, ABI.S_TASK + ABI.T_NCP].max() > 0          # the contact rows were exercised
    assert not np.any(f1 & _lib.FLAGS_FAULT_MASK) and not np.any(f0 & _lib.FLAGS_FAULT_MASK)
    assert np.array_equal(G1, G0)
    assert len(o1) == len(o0) == 7
    for a, b in zip(o1, o0):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_one_substep_agrees(lib_and_scene):
    A, md = lib_and_scene
    S = np.concatenate([reset_states(A, md, range(0, 5), 'random'), reset_states(A, md, range(20, 23), 'tremor')])
    G = []
    for split in (True, False):
        sim = make_sim(md, len(S), split)
        assert sim.dyn_split() == int(split)
        sim.set_state(S)
        sim.substep(0.01)
        G.append(sim.get_state())
        sim.close()
    assert np.array_equal(G[0], G[1])


def test_mask_holds_for_both_roles(lib_and_scene):
    from avr import _lib
    A, md = lib_and_scene
    n = 24
    S = reset_states(A, md, range(n))
    sim = make_sim(md, n, True)
    assert sim.dyn_split() == 1
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
    ref = make_sim(md, n, True)
    ref.set_state(S)
    ref.settle(2)
    assert np.array_equal(after[~keep], ref.get_state()[~keep])
    sim.close(); ref.close()


def test_resources_with_the_switch_on(lib_and_scene):
    A, md = lib_and_scene
    sim = make_sim(md, 4, True)
    assert sim.dyn_split() == 1
    ki = sim.kernel_info()
    assert set(ki) == {'pairs', 'narrowphase', 'a', 'b', 'task'}
    assert all(k['scratch_bytes'] == 0 for k in ki.values())
    assert ki['pairs']['lds_bytes'] <= 10240              # 16 blocks of either role per CU
    sim.close()
