"""FeedingJacoNew-v0 (feeding.py:168-246, the `new` branches) on the height variants of one handle:
random gender, impairment 'none', a new hipbone_to_mouth_height per episode from a 1 cm grid over
+-0.1 m around the gender's default (the reference draws it continuously: DESIGN section 8), waist
joints in +-10 deg, head joints in +-30 deg, arm joints 0, and the reference's clearance loop --
while min getClosestPoints(human, robot, 0.05) < 0.01 the human's joint draws are redrawn --
restated on the host with the device narrowphase and bounded.
"""
import json

import numpy as np
import pytest

from avr import _abi as ABI
from avr import model_compiler as MC
from avr import reset as RS


def test_height_grid_and_registration():
    from avr import env as EV
    G = EV.new_height_grid()
    for g in MC.GENDERS:
        h = np.array(G[g])
        assert len(h) == 21 and np.allclose(np.diff(h), 0.01) and abs(h[0] - (MC.DEFAULT_HEIGHT[g] - 0.1)) < 1e-12 and abs(h[-1] - (MC.DEFAULT_HEIGHT[g] + 0.1)) < 1e-12
        assert MC.DEFAULT_HEIGHT[g] in G[g]
    assert len(EV.variant_table(G)) == 42
    assert EV.is_built('FeedingJacoNew-v0') and EV.BUILT_ON['FeedingJacoNew-v0'] == 'FeedingJaco-v0'
    for k in EV.REGISTRY:
        if 'New' in k and k != 'FeedingJacoNew-v0':
            assert not EV.is_built(k), k
    with pytest.raises(NotImplementedError):
        EV.AVRVecEnv('FeedingPR2New-v0', 2)


def _rows(n=6):
    A = ABI.load_scene(ABI.TASK_FEEDING)
    md = ABI.ModelDesc(A)
    ids = list(range(n))
    S, _, _, _, meta = RS.reset_inputs(A, md, 1001, ids, impairment='none', stream='philox')
    return A, S, ids, [m['gender'] for m in meta]


def test_new_human_draws_are_in_range_and_keyed_by_redraw():
    A, S, ids, gl = _rows()
    eps = [0] * len(ids)
    Q0 = RS.new_human_rows(A, S.copy(), 1001, ids, eps, gl, 0)
    assert np.all(np.abs(Q0[:, 0:3]) <= np.deg2rad(10)) and np.all(np.abs(Q0[:, 25:28]) <= np.deg2rad(30))
    assert np.ptp(Q0[:, 0]) > 0 and np.ptp(Q0[:, 26]) > 0
    # the sitting angles and the arm joints (0 but for joints 10 and 20, whose first entry in the list
    # wins, world_creation.py:147-152) are FeedingJaco-v0's (feeding.py:229-231 = :242)
    base = RS.human_joint_angles_batch(A, 'male', Q0[:, 25:28], np.ones(len(ids)))
    rest = [j for j in range(base.shape[1]) if j not in (0, 1, 2)]
    for k, g in enumerate(gl):
        if g == 'male':
            np.testing.assert_array_equal(Q0[k, rest], base[k, rest])
    np.testing.assert_array_equal(Q0, RS.new_human_rows(A, S.copy(), 1001, ids, eps, gl, 0))
    Q1 = RS.new_human_rows(A, S.copy(), 1001, ids, eps, gl, 1)
    assert not np.any(Q0[:, 0:3] == Q1[:, 0:3])
    # keyed by the global env id: a shard draws what the batch draws
    np.testing.assert_array_equal(Q0[3:], RS.new_human_rows(A, S[3:].copy(), 1001, ids[3:], eps[3:], gl[3:], 0))
    mixed = RS.new_human_rows(A, S.copy(), 1001, ids, eps, gl, [0, 1, 0, 1, 0, 1])
    np.testing.assert_array_equal(mixed[0::2], Q0[0::2])
    np.testing.assert_array_equal(mixed[1::2], Q1[1::2])


def test_redraw_loop_advances_ends_and_is_bounded():
    """An injected distance function: 0.005 on the first attempt -> the human's draws advance to
    redraw 1 and the loop ends; always 0.005 -> the loop stops at the bound."""
    A, S, ids, gl = _rows()
    eps = [0] * len(ids)
    RS.new_human_rows(A, S, 1001, ids, eps, gl, 0)
    hs = slice(ABI.S_HUMAN, ABI.S_HUMAN + 7 * ABI.MAX_HUMAN)
    first = S.copy()
    calls = []

    def once(rows, genders):
        calls.append(len(rows))
        return np.full(len(rows), 0.005 if len(calls) == 1 else 0.03)

    W = S.copy()
    redraws, dist = RS.new_redraw_loop(A, W, 1001, ids, eps, gl, once)
    assert calls == [len(ids), len(ids)] and np.all(redraws == 1) and np.all(dist == 0.03)
    want = first.copy()
    RS.new_human_rows(A, want, 1001, ids, eps, gl, 1)
    np.testing.assert_array_equal(W, want)
    assert not np.array_equal(W[:, hs], first[:, hs])
    # only the envs that are too close redraw
    W = S.copy()
    redraws, _ = RS.new_redraw_loop(A, W, 1001, ids, eps, gl, lambda rows, g: np.where(np.arange(len(rows)) == 0, 0.005, 0.03) if len(rows) == len(ids) else np.full(len(rows), 0.02))
    assert redraws.tolist() == [1] + [0] * (len(ids) - 1)
    np.testing.assert_array_equal(W[1:], first[1:])
    # never clear: bounded
    n = []
    redraws, dist = RS.new_redraw_loop(A, S.copy(), 1001, ids, eps, gl, lambda rows, g: (n.append(1), np.full(len(rows), 0.005))[1])
    assert np.all(redraws == RS.NEW_REDRAWS) and len(n) == RS.NEW_REDRAWS + 1 and np.all(dist == 0.005)


def test_distance_function_asks_the_rows_slot_and_gender():
    """human_robot_distance: pairs are human shapes of the row's gender x robot shapes, each with the
    row's slot; the minimum over the hits, thr when nothing is within thr."""
    A, S, ids, gl = _rows(4)
    S[:, ABI.S_TASK + ABI.T_GENDER] = [2, 5, 0, 1]
    gl = ['male', 'female', 'male', 'female']
    seen = {}

    def fake(pairs, poses, thr, slots):
        seen.update(pairs=pairs, slots=slots, thr=thr)
        out = np.zeros((len(pairs), 8), np.float32)
        out[:, 0] = 1
        out[:, 7] = 0.04
        out[slots == 5, 7] = 0.002
        out[slots == 0, 0] = 0
        return out

    # the arm folded at q = 0 sits beside the human: some pairs survive the bounding-sphere cull
    d = RS.human_robot_distance(A, S, gl, fake)
    assert seen['thr'] == 0.05 and set(seen['slots']) == {0, 1, 2, 5}
    hg = A['shape_gender'][seen['pairs'][:, 0]]
    assert np.all(A['body_kind'][A['shape_body'][seen['pairs'][:, 0]]] == ABI.BODY_HUMAN)
    assert np.all(A['body_kind'][A['shape_body'][seen['pairs'][:, 1]]] == ABI.BODY_ROBOT)
    for slot, g in ((2, 0), (5, 1), (0, 0), (1, 1)):
        assert np.all((hg[seen['slots'] == slot] == g) | (hg[seen['slots'] == slot] < 0))
    np.testing.assert_allclose(d, [0.04, 0.002, 0.05, 0.04])


# --------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope='module')
def new_env():
    from avr import env as EV
    v = EV.AVRVecEnv('FeedingJacoNew-v0', 8, auto_reset=False, prefetch=False)
    yield v
    v.close()


@pytest.mark.gpu
def test_reset_draws_a_person_per_env_and_episode(new_env):
    v = new_env
    L = v.L
    assert len(v.variants) == 42 and v.sim.human_variants() == [(MC.GENDERS.index(g), pytest.approx(h, abs=1e-6)) for g, h in v.variants]
    obs0 = v.reset()
    S0 = v.get_state()
    genders, heights = v.proportions(S0)
    assert set(genders) == {'male', 'female'}
    for g, h in zip(genders, heights):
        assert abs(h - MC.DEFAULT_HEIGHT[g]) <= 0.1 + 1e-9 and abs(h * 100 - round(h * 100)) < 1e-9
    assert len(set(heights)) > 2
    assert np.all(S0[:, L.S_TASK + L.T_HDYN] == 0)                                       # impairment 'none'
    assert np.all(S0[:, L.S_TASK + L.T_GENDER] >= 2)
    assert np.all(v.last_human_robot_distance >= 0.01)
    d = RS.human_robot_distance(v.A, S0.astype(np.float64), genders, v.sim.narrowphase)
    assert np.all(d >= 0.01), d
    assert v.reset_timing['human_redraws'] >= 0 and v.reset_timing['human_redraws_max'] <= RS.NEW_REDRAWS
    z = S0[:, L.S_TASK + L.T_TARGET + 2]
    assert np.ptp(z) > 0.01, z
    assert np.all(np.isfinite(obs0)) and np.all(v.flags() & 0x1f == 0)
    # the waist angles: the waist link's rotation away from upright is at most the three +-10 deg joints'
    ids = list(range(8))
    Q = RS.new_human_rows(v.A, S0.astype(np.float64), v.seed, ids, [0] * 8, genders, 0, v._variant_ctx)
    assert np.all(np.abs(Q[:, 0:3]) <= np.deg2rad(10))
    if v.reset_timing['human_redraws'] == 0:
        W = S0.astype(np.float64)
        RS.new_human_rows(v.A, W, v.seed, ids, [0] * 8, genders, 0, v._variant_ctx)
        hs = slice(L.S_HUMAN, L.S_HUMAN + 7 * L.MAX_HUMAN)
        np.testing.assert_allclose(S0[:, hs], W[:, hs], atol=1e-6)
    # a second episode redraws the person
    v.episode += 1
    v.reset()
    g1, h1 = v.proportions()
    assert (g1, h1.tolist()) != (genders, heights.tolist())
    v.episode[:] = 0


@pytest.mark.gpu
def test_free_space_steps_track_per_height_oracles(new_env):
    """20 gym steps from the env's own reset with the food and the bowl moved away (free space, as
    test_vec_env_at_odd_height_tracks_oracle): within 1e-3 rad of the fp64 oracle on each env's
    height's scene."""
    from avr import _lib
    from oracle.oracle import Oracle
    v = new_env
    L = v.L
    v.reset()
    S = v.get_state().copy()
    for f in range(1, ABI.MAX_FREE):
        b = ABI.S_FREE + ABI.FB_WORDS * f
        S[:, b:b + 3] = [60.0 + 3 * f, 60.0, 500.0]
        S[:, b + 3:b + 7] = [0, 0, 0, 1]
        S[:, b + 7:b + 13] = 0
    v.set_state(S)
    genders, heights = v.proportions(S)
    oracles = []
    for e in range(v.n):
        md_h = ABI.ModelDesc(MC.scene_arrays('feeding_jaco', {genders[e]: heights[e]}))
        o = Oracle(md_h, 1)
        row = S[e:e + 1].astype(np.float64)
        row[0, L.S_TASK + L.T_GENDER] = MC.GENDERS.index(genders[e])
        o.set_state(row)
        oracles.append(o)
    worst = 0.0
    for t in range(20):
        a = _lib.random_actions(1001, np.arange(v.n), t)
        v.step(a)
        G = v.get_state()
        for e, o in enumerate(oracles):
            o.step(a[e:e + 1])
            worst = max(worst, np.abs(G[e, :v.md.n_dof] - o.get_state()[0, :v.md.n_dof]).max())
    assert worst < 1e-3, worst


@pytest.mark.gpu
def test_recording_replays_with_the_real_heights(new_env, tmp_path):
    from avr import _lib
    from avr import record as R
    v = new_env
    rec = R.Recorder(v, str(tmp_path / 'rec'))
    rec.reset()
    genders, heights = v.proportions()
    for t in range(3):
        rec.step(_lib.random_actions(1001, np.arange(v.n), t))
    rec.close()
    setup = json.load(open(str(tmp_path / 'rec' / 'setup.json')))
    assert setup['gender'] == genders and setup['hipbone_to_mouth_height'] == pytest.approx(heights.tolist())
    assert setup['human_heights'] == {g: [pytest.approx(h) for h in hs] for g, hs in v.human_heights_arg.items()} and len(setup['human_heights']['male']) == 21
    rp = R.ReplayEnv(str(tmp_path / 'rec'))
    rp.reset()
    for t in range(3):
        rp.step()
    assert rp.mismatch == []
    assert rp.env.proportions()[1].tolist() == pytest.approx(heights.tolist())
    rp.close()


@pytest.mark.gpu
def test_reset_pool_rows_carry_mixed_slots():
    """reset_pool=m with the New id: the pool is built through this reset, so its rows carry mixed
    slots, and a rolled-over env steps on as the person of its pool row."""
    import torch
    from avr import env as EV
    v = EV.AVRTorchVecEnv('FeedingJacoNew-v0', 4, prefetch=False, reset_pool=2)
    v.reset()
    L = v.L
    S = v.get_state()
    S[:, L.S_TASK + L.T_ITER] = v.max_steps - 1
    v.set_state(S)
    a = torch.zeros(4, 7, device='cuda')
    _, _, done, _ = v.step(a)
    assert bool(done.all())
    R = v.get_state()
    slots = R[:, L.S_TASK + L.T_GENDER]
    assert np.all(slots >= 2) and np.all(R[:, L.S_TASK + L.T_ITER] == 0)
    v.step(a)
    assert np.all(v.flags() & 0x1f == 0)
    v.close()
