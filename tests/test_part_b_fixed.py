"""Part B's fixed costs (B4_FIXED, FeedingJaco's default): on the LDS row sources the active list
reads a group's normal impulses before its first ballot, and the non-contact sweep of the next
iteration starts its reads during the current one, to be issued again when a group converges.
Neither may change a bit: the global-row path (AVR_B4_GLOBAL=1) keeps the earlier code and is the
reference, as in test_part_b_sweeps.py, whose helpers these tests use.  The PR2 tasks build with the
switch off (they lose with it); their cases hold for either setting (-DB4_FIXED=1 builds pass them).

FeedingJaco states: tests/golden/part_b_fixed_feeding.npz (tools/make_part_b_fixed_fixture.py, the
fp64 oracle on the CPU): 37 envs, so the blocks after the first eight hold one live env and three
past the end, or none; contact-rich states 29 random gym steps into the episode; every third env
its raw reset state without bowl and food (no contact); env 1 with about 66 contacts in one block
with env 9 (none) and env 17 (a few): the staging loop (16 lanes x 8 loads of 16 bytes per group
and round, 3 records of 64 bytes per contact) runs six rounds for the first, none for the second
and one for the third, and a loop 32 loads deep (measured, not kept) would run two for the first.
"""
import os

import numpy as np
import pytest

import test_part_b_sweeps as T
from test_part_b_sweeps import GLB, LDS, lib_and_scene, make_sim, same, same_outs  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'part_b_fixed_feeding.npz')
N = 37
EMPTIED = tuple(range(0, N, 3))


@pytest.fixture(scope='module')
def feeding_states(lib_and_scene):
    """The fixture's states, with the oracle's contact counts of their first sub-step."""
    from avr import _abi as ABI
    from oracle.oracle import Oracle
    A, md = lib_and_scene
    S = np.load(GOLDEN)['S']
    assert S.shape == (N, ABI.STATE_WORDS) and S.dtype == np.float32
    o = Oracle(md, N)
    o.set_state(S.astype(np.float64))
    o.substep(0.01)
    ncp = o.get_state()[:, ABI.S_TASK + ABI.T_NCP].astype(int)
    o.close()
    return S, ncp


def test_states_fill_the_blocks_unevenly(feeding_states):
    """The oracle's contact counts of the first sub-step: the emptied envs have none, and some block
    holds an env with 43 or more contacts (more than 32 staging loads per lane) beside one with
    fewer than 11 (one round of 8 loads; not an emptied env) and beside an empty one."""
    S, ncp = feeding_states
    print('oracle contacts per env:', ncp.tolist())
    assert np.all(ncp[list(EMPTIED)] == 0)
    assert np.count_nonzero(ncp >= 20) >= 20
    blocks = [ncp[x:32:8] for x in range(8)]
    assert any(b.max() >= 43 and np.any((b > 0) & (b < 11)) and np.any(b == 0) for b in blocks)
    assert ncp[1] >= 43 and 0 < ncp[17] < 11 and ncp[9] == 0


def _substep(md, S, path):
    from avr import _abi as ABI
    G, F = T._substep(md, S, path)
    return G, F, G[:, ABI.S_TASK + ABI.T_NCP].astype(int)


def test_feeding_one_substep_agrees(lib_and_scene, feeding_states):
    A, md = lib_and_scene
    S, ncp = feeding_states
    G0, F0, n0 = _substep(md, S, GLB)
    G, F, n = _substep(md, S, LDS)
    print('contacts per env:', n.tolist())
    # the kernels' own counts: the same uneven block as the oracle's
    assert n[1] >= 43 and 0 < n[17] < 11 and np.all(n[list(EMPTIED)] == 0)
    assert same(G, G0) and np.array_equal(F, F0)


def _steps(md, S, path, k=3):
    from avr import _lib
    n = len(S)
    sim = make_sim(md, n, path)
    sim.set_state(S)
    outs = [sim.step(_lib.random_actions(1001, np.arange(n), 40 + j)) for j in range(k)]
    G, F = sim.get_state(), sim.get_flags()
    sim.close()
    return G, outs, F


def test_feeding_three_steps_agree(lib_and_scene, feeding_states):
    from avr import _lib
    A, md = lib_and_scene
    S, _ = feeding_states
    G0, o0, F0 = _steps(md, S, GLB)
    G, o, F = _steps(md, S, LDS)
    assert not np.any(F0 & _lib.FLAGS_FAULT_MASK)
    assert same(G, G0) and np.array_equal(F, F0)
    assert len(o) == 3 and same_outs(o, o0)


def test_feeding_masked_reset_agrees(lib_and_scene, feeding_states):
    """Three steps, then a reset of all but envs 8, 24, 1 and 17 with two settle frames: the heavy
    env 1 and the light env 17 of block 1 are masked off and run null rows beside live ones."""
    A, md = lib_and_scene
    S, _ = feeding_states
    mask, b0, a0, obs0, f0 = T._masked(md, S, GLB)
    _, b1, a1, obs1, f1 = T._masked(md, S, LDS)
    keep = mask == 0
    assert same(a1[keep], b1[keep])
    assert same(b1, b0) and same(a1, a0) and same(obs1, obs0) and np.array_equal(f1, f0)


@pytest.mark.parametrize('task', ['scratch', 'bedbath'])
def test_pr2_tasks_agree_with_early_exits(lib_and_scene, task):
    """The PR2 tasks, 8 reset states and their pressed-tool copies, three gym steps: their groups
    converge at different iterations (the oracle's PGS runs fewer iterations than solves x
    solver_iterations), so reads issued ahead for a group that then converges are issued again,
    with the other groups of its wave still sweeping."""
    from avr import _abi as ABI, _lib
    from oracle.oracle import Oracle
    t = ABI.TASK_SCRATCH if task == 'scratch' else ABI.TASK_BEDBATH
    md, S = T._pr2_states(t, 8)
    n = len(S)
    assert n > 8
    o = Oracle(md, n)
    o.set_state(S.astype(np.float64))
    o.step(_lib.random_actions(1001, np.arange(n), 0) * 0.5)
    st = o.stats()
    o.close()
    iters = int(md.desc.solver_iterations)
    print('oracle PGS: %d iterations in %d solves of at most %d' % (st[3], st[4], iters))
    assert st[4] > 0 and 0 < st[3] < st[4] * iters          # some solve leaves before iters ...
    assert st[3] > st[4]                                    # ... and not every one after its first
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
    assert ncp0 > 0 and ncp == ncp0
    assert same(G, G0) and np.array_equal(f, f0)
    assert same_outs(o, o0)
