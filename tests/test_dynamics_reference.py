"""The oracle's articulated dynamics against an independent Lagrangian forward dynamics
(tests/dyn_reference.py: Jacobian mass matrix, Christoffel bias from differences of M, numpy
float64) away from the rest state, on the three robot models, and the conditions under which
tests/test_gpu_dynamics.py holds the kernel to the fp64 oracle (tests/dyn_util.py: states, filter,
rule).  The chain is: Lagrangian reference -> fp64 oracle -> kernel.

Measured here (printed by the tests):
  * oracle vs reference, worst |(qd' - qd) - dt qdd_ref| / max|dt qdd_ref| over 32 contact-free
    free states per task: FeedingJaco 7.8e-8, ScratchItchPR2 1.7e-7, BedBathingPR2 3.2e-7
    (bound 1e-5: difference-quotient and conditioning error; cond(M) up to 3.6e4 / 3.5e5);
  * kept envs free / limit / clamp / driven: FeedingJaco 70 / 47 / 58 / 36 of 192 / 192 / 192 / 48,
    ScratchItchPR2 58 / 57 / 58 / 32 of 64 / 64 / 64 / 32, BedBathingPR2 79 / 85 / - / 8 of
    96 / 96 / - / 8;
  * share of envs with E32 > 8 s: robot block at most 0.063, chain block at most 0.085 (all
    words together: 0.138 in ScratchItchPR2 free, at most 0.07 elsewhere; dyn_util's docstring).
"""
import numpy as np
import pytest

import dyn_reference as R
import dyn_util as U

TASKS = ['feeding', 'scratch', 'bedbath']
ORACLE_TOL = 1e-5


@pytest.fixture(scope='module', autouse=True)
def _oracle(oracle_built):
    return True


# ----------------------------------------------------------------------------- the reference itself
def _double_pendulum():
    import kat_scene as K
    m1, m2, l1, l2, I = 1.0, 0.7, 0.4, 0.3, 1e-3
    links = [dict(parent=-1, axis=[1, 0, 0], jpos=[0, 0, 1], com_pos=[0, 0, -l1], mass=m1, inertia=[I, I, I]),
             dict(parent=0, axis=[1, 0, 0], jpos=[0, 0, -l1], com_pos=[0, 0, -l2], mass=m2, inertia=[I, I, I])]
    return K.chain_scene(links), (m1, m2, l1, l2, I)


def test_reference_matches_planar_double_pendulum():
    """M and c of the chain of test_double_pendulum_energy_drift against the textbook closed form
    (point masses at l1 and l2 plus I about the axis; link 1's COM is joint 2)."""
    A, (m1, m2, l1, l2, I) = _double_pendulum()
    base = np.array([0, 0, 0, 0, 0, 0, 1.0])
    rng = np.random.default_rng(5)
    for _ in range(8):
        q, qd = rng.uniform(-3, 3, 2), rng.uniform(-3, 3, 2)
        c2, s2 = np.cos(q[1]), np.sin(q[1])
        M = np.array([[m1 * l1 ** 2 + m2 * (l1 ** 2 + l2 ** 2 + 2 * l1 * l2 * c2) + 2 * I, m2 * (l2 ** 2 + l1 * l2 * c2) + I],
                      [m2 * (l2 ** 2 + l1 * l2 * c2) + I, m2 * l2 ** 2 + I]])
        c = m2 * l1 * l2 * s2 * np.array([-(2 * qd[0] * qd[1] + qd[1] ** 2), qd[0] ** 2])
        assert np.allclose(R.mass_matrix(A, q, base), M, rtol=0, atol=1e-14)
        assert np.allclose(R.bias(A, q, qd, base), c, rtol=0, atol=1e-9 * (1 + np.abs(c).max()))


@pytest.mark.parametrize('name', TASKS)
def test_reference_mass_matrix_spd_and_energy_identity(name):
    """M is symmetric positive definite, and qd^T c = 1/2 qd^T Mdot qd (the velocity-product forces
    do no net work beyond the change of M), with Mdot from a central difference of M along qd, a
    difference the Christoffel sum does not use."""
    t = U.task(name)
    sc = U.scenario(name, 'free')
    S = sc['S'][np.nonzero(sc['keep'])[0][:6]]
    for st in S:
        q, qd, base = st[t.L.S_Q:t.L.S_Q + t.nd], st[t.L.S_QD:t.L.S_QD + t.nd], t.base_pose(st)
        M = R.mass_matrix(t.A, q, base)
        assert np.abs(M - M.T).max() <= 1e-15 * np.abs(M).max()
        assert np.linalg.eigvalsh(M).min() > 0
        h = 1e-6
        Mdot = (R.mass_matrix(t.A, q + h * qd, base) - R.mass_matrix(t.A, q - h * qd, base)) / (2 * h)
        power = 0.5 * qd @ Mdot @ qd
        scale = np.abs(np.outer(qd, qd) * Mdot).sum()
        assert abs(qd @ R.bias(t.A, q, qd, base) - power) <= 1e-7 * scale


# ----------------------------------------------------------------------------- oracle vs reference
@pytest.mark.parametrize('name', TASKS)
def test_oracle_substep_matches_lagrangian_reference(name):
    """32 kept free states, damping off: the fp64 oracle's qd' - qd of the robot DoFs after one
    sub-step is dt qdd_ref to 1e-5 of max|dt qdd_ref| per env (poses anywhere inside the limits,
    velocities +-3 on every DoF, so every velocity-product term of the bias forces is at work).
    Measured worst: FeedingJaco 7.8e-8, ScratchItchPR2 1.7e-7, BedBathingPR2 3.2e-7 (1e-5 is 30 x
    the worst, and four orders below what a wrong term gives)."""
    t = U.task(name)
    L, nd = t.L, t.nd
    sc = U.scenario(name, 'free')
    S = sc['S'][np.nonzero(sc['keep'])[0][:32]]
    assert len(S) == 32
    C = U.oracle_substep(t.md_nodamp, S, t.dt, 'f64')
    dev, cond = np.zeros(len(S)), np.zeros(len(S))
    for e, st in enumerate(S):
        qd = st[L.S_QD:L.S_QD + nd]
        qdd, M, _ = R.forward_dynamics(t.A, st[L.S_Q:L.S_Q + nd], qd, t.base_pose(st))
        dev[e] = np.abs(C[e, L.S_QD:L.S_QD + nd] - qd - t.dt * qdd).max() / np.abs(t.dt * qdd).max()
        cond[e] = np.linalg.cond(M)
    print('%s: oracle vs Lagrangian reference, worst relative deviation of dt qdd %.3g (cond(M) up to %.3g)' % (name, dev.max(), cond.max()))
    assert np.all(dev <= ORACLE_TOL), dev


def _limit_envs(t, sc):
    """(env, DoF, side, inward sign, erp pen / dt) of the kept limit envs."""
    erp = t.md.params['erp']
    out = []
    for e in np.nonzero(sc['keep'])[0]:
        d, side = U.limit_case(t, e)
        q = sc['S'][e, t.L.S_Q + d]
        pen = t.lower[d] - q if side == 0 else q - t.upper[d]
        assert 0.0099 < pen < 0.0101
        out.append((int(e), d, side, 1.0 if side == 0 else -1.0, erp * pen / t.dt))
    return out


@pytest.mark.parametrize('name', TASKS)
def test_oracle_limit_row_closed_form(name):
    """A kept limit env's pushed DoF leaves the sub-step with inward velocity >= erp pen / dt (pen:
    the state's own excursion, 0.01 rounded to fp32 with q).  Where the reference's unconstrained
    velocity violates that, the row -- alone, the motor rows capped at zero -- is met exactly (1e-12);
    elsewhere (light gripper DoFs whose bias term alone exceeds the target) the larger inward
    velocity stays.  Damping off, so that the reference's unconstrained velocity is the oracle's."""
    t = U.task(name)
    L, nd = t.L, t.nd
    sc = U.scenario(name, 'limit')
    C = U.oracle_substep(t.md_nodamp, sc['S'], t.dt, 'f64')
    n_eq = n_free = 0
    worst = 0.0
    for e, d, side, sg, target in _limit_envs(t, sc):
        st = sc['S'][e]
        inward = sg * C[e, L.S_QD + d]
        assert inward >= target - 1e-12, (e, d, side, inward, target)
        qdd, _, _ = R.forward_dynamics(t.A, st[L.S_Q:L.S_Q + nd], st[L.S_QD:L.S_QD + nd], t.base_pose(st))
        unc = sg * (st[L.S_QD + d] + t.dt * qdd[d])
        if unc < target - 1e-4:                           # (1e-4: far above the reference's own error)
            assert abs(inward - target) <= 1e-12, (e, d, side, inward, target)
            worst = max(worst, abs(inward - target))
            n_eq += 1
        elif unc > target + 1e-4:
            n_free += 1
    print('%s: limit row met exactly on %d kept envs (worst %.3g), left alone on %d' % (name, n_eq, worst, n_free))
    assert n_eq >= sc['keep'].sum() // 2


# ----------------------------------------------------------------------------- the rule's conditions
@pytest.mark.parametrize('name', TASKS)
def test_filter_keeps_enough_and_fp32_errors_are_not_heavy_tailed(name):
    """What the GPU file relies on, from the two oracles alone: free, limit (and clamp) keep at
    least 32 envs, driven at least half; every limited DoF and both sides appear among the kept
    limit envs; per block at most 1/8 of the envs have E32 > 8 s."""
    t = U.task(name)
    for kind in ('free', 'limit', 'clamp', 'driven'):
        if kind == 'clamp' and name == 'bedbath':
            continue
        sc = U.scenario(name, kind)
        k, kc = sc['keep'], sc['keep_chain']
        b64, b32 = U.blocks(t, kind, sc['C64']), U.blocks(t, kind, sc['C32'])
        a64, a32 = U.compared(t, kind, sc['C64']), U.compared(t, kind, sc['C32'])
        share = dict(all=U.outlier_share(a64[k], a32[k]), robot=U.outlier_share(b64['robot'][k], b32['robot'][k]))
        if t.nc:
            share['chain'] = U.outlier_share(b64['chain'][kc], b32['chain'][kc])
        r = U.rule(b64['robot'][k], b32['robot'][k], b32['robot'][k])
        print('%s %s: kept %d (chain block %d) of %d; fp32 oracle robot-block error median %.3g worst %.3g; share of envs with E32 > 8 s %s'
              % (name, kind, k.sum(), kc.sum(), len(k), r['s'], r['E32'].max(), {b: round(v, 3) for b, v in share.items()}))
        assert k.sum() >= (len(k) + 1) // 2 if kind == 'driven' else k.sum() >= 32
        if t.nc:
            assert kc.sum() >= (len(k) + 1) // 2 if kind == 'driven' else kc.sum() >= 32
        assert share['robot'] <= 0.125
        assert share.get('chain', 0.0) <= 0.125
        if kind == 'limit':
            seen = {U.limit_case(t, e) for e in np.nonzero(k)[0]}
            assert seen == {(int(d), s) for d in t.limited for s in (0, 1)}
        if kind == 'clamp':                              # DoF 0 leaves at the clamp in both oracles
            print('  DoF 0 clamped in both oracles: %d of the kept' % U.clamped_in_both(t, sc).sum())
            assert U.clamped_in_both(t, sc).sum() >= 32


def _rejected(t, kind, sc, Xg):
    k = sc['keep']
    b64, b32, bg = (U.blocks(t, kind, X[k])['robot'] for X in (sc['C64'], sc['C32'], Xg))
    return U.rule(b64, b32, bg)['ratio']


@pytest.mark.parametrize('name', TASKS)
def test_rule_rejects_permuted_inertia_axes(name):
    """The "device" is the fp32 oracle with the principal inertias of one arm link (arm DoF 3's)
    cycled: a plausible-looking arm.  The rule rejects it on most envs (measured: median ratio
    Eg / bound FeedingJaco 2.4e3, ScratchItchPR2 80, BedBathingPR2 88); the unaltered fp32 oracle
    passes by construction (ratio <= 1/8)."""
    from avr import _abi as ABI
    t = U.task(name)
    sc = U.scenario(name, 'free')
    A2 = dict(t.A)
    l = t.dof_link[t.md.arm_dofs[3]]
    I = np.array(t.A['rl_inertia'], np.float64)
    assert np.ptp(I[l]) > 0.2 * I[l].max()                # distinct principal inertias
    I[l] = np.roll(I[l], 1)
    A2['rl_inertia'] = I
    Xg = U.oracle_substep(ABI.ModelDesc(A2, U.FREE_PARAMS), sc['S'], t.dt, 'f32')
    ratio = _rejected(t, 'free', sc, Xg)
    print('%s: permuted inertia axes, Eg / bound median %.3g max %.3g' % (name, np.median(ratio), ratio.max()))
    assert _rejected(t, 'free', sc, sc['C32']).max() <= 0.125
    assert np.median(ratio) > 10


@pytest.mark.parametrize('name', TASKS)
def test_rule_rejects_lost_velocity_products(name):
    """The "device" is the fp32 oracle fed qd = 0 with qd added back afterwards: what a kernel
    whose Coriolis, centrifugal and gyroscopic terms (and |v| damping) were lost would return.
    Measured: median ratio Eg / bound FeedingJaco 4.7e4, ScratchItchPR2 2.7e4, BedBathingPR2 3.2e4."""
    t = U.task(name)
    L, n = t.L, t.nd + t.nc
    sc = U.scenario(name, 'free')
    S0 = sc['S'].copy()
    S0[:, L.S_QD:L.S_QD + L.MAX_DOF] = 0.0
    Xg = U.oracle_substep(sc['md'], S0, t.dt, 'f32')
    Xg[:, L.S_QD:L.S_QD + n] += sc['S'][:, L.S_QD:L.S_QD + n]
    Xg[:, L.S_Q:L.S_Q + n] = sc['S'][:, L.S_Q:L.S_Q + n] + t.dt * Xg[:, L.S_QD:L.S_QD + n]
    ratio = _rejected(t, 'free', sc, Xg)
    print('%s: velocity products lost, Eg / bound median %.3g max %.3g' % (name, np.median(ratio), ratio.max()))
    assert np.median(ratio) > 10
