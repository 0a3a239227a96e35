"""GPU: device-side episode rollover from a reset-state pool (csrc/avr_rollover.hip, include/avr.h
avr_reset_pool_set / avr_rollover_*): rollouts with the rollover mode on against the host loop of
single calls, set_state_masked and _lib.rollover_index, bit for bit, in both replay forms, the
direct loop, all three multi-kernel tasks; the mode-off graphs untouched; pool replacement without
re-capture; the error paths and the torch facade.

Episodes are made to end inside a short rollout by staging T_ITER (done is exactly T_ITER >=
max_steps after the step's increment): an env staged to max_steps - d finishes at slot d - 1.  Pool
rows are data too: some carry T_ITER = max_steps - 3, so an env that takes one finishes again three
steps later and rolls over a second time, with episode = 1."""
import numpy as np
import pytest

from test_gpu_policy import _rollout, _stacked, feeding, make_sim, policy25      # noqa: F401 (fixtures)
from test_policy_host import random_policy

pytestmark = pytest.mark.gpu

SEED = 1001
D7 = (1, 2, 15, 16, 17, 19, None)      # steps to an env's first done, cycled over the envs (None: never)


def dev_tensor(ptr, shape, typestr):
    """A torch tensor over device memory the handle owns (no copy)."""
    import torch
    holder = type('_DevArray', (), {})()
    holder.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)
    return torch.as_tensor(holder, device='cuda')


def rollover_rows(sim):
    """Host copies of the handle's (term_obs, term_value, episode) rows."""
    to, tv, ep = sim.rollover_buffers()
    sim.sync()
    return (dev_tensor(to, (sim.n, sim.obs_dim), '<f4').cpu().numpy(), dev_tensor(tv, (sim.n,), '<f4').cpu().numpy(),
            dev_tensor(ep, (sim.n,), '<i4').cpu().numpy())


def stage(md, S, D):
    """Copy of S with env e's T_ITER at max_steps - D[e % len(D)] (None: left alone)."""
    L, ms = md.layout, int(md.params['max_episode_steps'])
    S = np.array(S, np.float32)
    for e in range(len(S)):
        d = D[e % len(D)]
        if d is not None:
            S[e, L.S_TASK + L.T_ITER] = ms - d
    return S


def make_pool(md, S, rows, staged):
    """(pool states, pool observations): rows of S, the last `staged` of them with T_ITER = max_steps - 3;
    the observations are those a handle computes for the rows (settle(0))."""
    L, ms = md.layout, int(md.params['max_episode_steps'])
    P = np.array(S[list(rows)], np.float32)
    P[len(P) - staged:, L.S_TASK + L.T_ITER] = ms - 3
    sim = make_sim(md, len(P))
    sim.set_state(P)
    O = sim.settle(0)
    sim.close()
    return P, O


def plan(md, S, P, K, env_offset=0, episodes=None):
    """The rollovers K steps must produce, from the T_ITER arithmetic and the host mirror alone:
    (envs done per slot [K], final episode counters, rollovers per env)."""
    L, ms = md.layout, int(md.params['max_episode_steps'])
    from avr import _lib
    it = S[:, L.S_TASK + L.T_ITER].astype(np.int64)
    pit = P[:, L.S_TASK + L.T_ITER].astype(np.int64)
    ep = np.zeros(len(S), np.int64) if episodes is None else np.array(episodes, np.int64)
    per_slot, rolls = [], np.zeros(len(S), np.int64)
    for _ in range(K):
        it += 1
        idx = np.nonzero(it >= ms)[0]
        per_slot.append(len(idx))
        if len(idx):
            it[idx] = pit[_lib.rollover_index(SEED, env_offset + idx, ep[idx], len(P))]
            ep[idx] += 1
            rolls[idx] += 1
    return np.array(per_slot), ep, rolls


def host_rollover(sim, done, obs_t, P, O, ep, term, env_offset=0):
    """The reference rollover of the envs with done set: pool rows picked by the host mirror land through
    set_state_masked, the observation rows (a device tensor) are overwritten, ep / term updated in place."""
    import torch
    from avr import _lib
    idx = np.nonzero(done)[0]
    if not len(idx):
        return
    j = _lib.rollover_index(SEED, env_offset + idx, ep[idx], len(P))
    term[idx] = obs_t[torch.from_numpy(idx).cuda()].cpu().numpy()
    St = np.zeros((sim.n, sim.words), np.float32)
    St[idx] = P[j]
    sim.set_state_masked(done.astype(np.uint8), St)
    obs_t[torch.from_numpy(idx).cuda()] = torch.from_numpy(O[j]).cuda()
    ep[idx] += 1


def loop_policy(sim, t0, K, obs0, det, B, P, O, ep, env_offset=0):
    """K x {policy_act_device; step_device; the host reads done and rolls the finished envs over} into
    the stacked layout; returns the terminal observations [E, obs_dim]."""
    import torch
    from avr import _abi as ABI
    n = sim.n
    term = np.zeros((n, sim.obs_dim), np.float32)
    o, r, i = torch.zeros(n, sim.obs_dim, device='cuda'), torch.zeros(n, device='cuda'), torch.zeros(n, ABI.INFO_DIM, device='cuda')
    dn = torch.zeros(n, dtype=torch.uint8, device='cuda')
    B['obs'][0].copy_(obs0)
    torch.cuda.synchronize()
    for k in range(K):
        sim.policy_act_device(t0 + k, B['obs'][k].data_ptr(), det, B['act'][k].data_ptr(), B['logp'][k].data_ptr(), B['value'][k].data_ptr())
        sim.step_device(B['act'][k].data_ptr(), o.data_ptr(), r.data_ptr(), dn.data_ptr(), i.data_ptr())
        sim.sync()
        host_rollover(sim, dn.cpu().numpy() != 0, o, P, O, ep, term, env_offset)
        B['obs'][k + 1].copy_(o); B['rew'][k].copy_(r); B['done'][k].copy_(dn); B['info'][k].copy_(i)
        torch.cuda.synchronize()
    sim.policy_act_device(t0 + K, B['obs'][K].data_ptr(), det, None, None, B['value'][K].data_ptr())
    sim.sync()
    return term


def term_values(sim, term):
    """policy_act_device's value on the terminal rows."""
    import torch
    t = torch.from_numpy(term).cuda()
    v = torch.zeros(sim.n, device='cuda')
    torch.cuda.synchronize()
    sim.policy_act_device(0, t.data_ptr(), True, None, None, v.data_ptr())
    sim.sync()
    return v.cpu().numpy()


def check_policy_identity(md, S, P, O, desc, groups, K, t0=5, det=False, env_offset=0, graph=True):
    """Handle A: rollover mode on, one stacked policy rollout.  Handle B: the host loop.  Everything equal,
    bit for bit; returns (A's stacked outputs, the plan) for further assertions."""
    import torch
    n = len(S)
    a, b = (make_sim(md, n, env_offset=env_offset) for _ in range(2))
    assert a.env_groups() == groups and b.env_groups() == groups
    for s in (a, b):
        s.set_state(S)
        obs0 = s.settle(2)
        s.policy_set(desc)
        s.reset_pool_set(P, O)
    S0 = a.get_state()                       # (settle frames do not touch T_ITER: the plan holds)
    per_slot, ep_plan, rolls = plan(md, S0, P, K, env_offset)
    a.rollover_enable(True)
    obs0 = torch.from_numpy(obs0).cuda()
    Ba, Bb = _stacked(n, K, md.layout.OBS_DIM), _stacked(n, K, md.layout.OBS_DIM)
    torch.cuda.synchronize()
    c0 = a.graph_captures()
    _rollout(a, t0, K, obs0, det, Ba)
    a.sync()
    if graph:
        assert a.graph_captures() == c0 + 1              # (one rollout graph set; the graph path ran)
    else:
        assert a.graph_captures() <= c0 + 1              # (at most the single step's graph)
    ep = np.zeros(n, np.int64)
    term = loop_policy(b, t0, K, obs0, det, Bb, P, O, ep, env_offset)
    torch.cuda.synchronize()
    # the reference loop did what was planned (it cannot pass vacuously) ...
    assert np.array_equal(Bb['done'].cpu().numpy().sum(1), per_slot) and np.array_equal(ep, ep_plan)
    # ... and the device rollover equals it
    assert np.array_equal(a.get_state(), b.get_state())
    for k in Ba:
        assert torch.equal(Ba[k], Bb[k]), k
    to, tv, de = rollover_rows(a)
    assert np.array_equal(to, term) and np.array_equal(de, ep)
    assert np.array_equal(tv, term_values(b, term))
    assert np.all(to[rolls == 0] == 0) and np.all(np.any(to[rolls > 0] != 0, axis=1))
    out = {k: v.cpu().numpy() for k, v in Ba.items()}
    a.close()
    b.close()
    return out, (per_slot, ep_plan, rolls)


@pytest.fixture(scope='module')
def feeding_obs16(feeding):
    """The observations of the module's 16 reset states (settle(0) on one handle), computed once."""
    A, md, S = feeding
    sim = make_sim(md, len(S))
    sim.set_state(S)
    O = sim.settle(0)
    sim.close()
    O.setflags(write=False)
    return O


def pick_pool(md, S, O16, rows, staged):
    """make_pool from rows of the module's states and their observations (no handle needed: the pool's
    observations are data, and the staged rows keep their state's observation)."""
    L, ms = md.layout, int(md.params['max_episode_steps'])
    P = np.array(S[list(rows)], np.float32)
    P[len(P) - staged:, L.S_TASK + L.T_ITER] = ms - 3
    return P, np.array(O16[list(rows)], np.float32)


@pytest.fixture(scope='module')
def feeding_pool(feeding, feeding_obs16):
    """(pool states, observations) of 5 rows from the module's reset states: 2 with T_ITER = 0, 3 staged to
    max_steps - 3; never modified."""
    A, md, S = feeding
    P, O = pick_pool(md, S, feeding_obs16, (3, 7, 11, 2, 9), 3)
    P.setflags(write=False)
    O.setflags(write=False)
    return P, O


@pytest.mark.parametrize('mode', ['groups', 'branches'])
def test_rollover_equals_host_loop_feeding(feeding, feeding_pool, policy25, mode, monkeypatch):
    """FeedingJaco (1900 words: the 16-byte copy), 80 envs in 3 groups (32 / 32 / 16), K = 19 (a 16-step
    chunk plus three remainder replays), first rollovers at slots 0, 1, 14, 15, 16, 18 spread over
    every group with envs 31, 32 and 79 (group edges) finishing."""
    monkeypatch.setenv('AVR_ENV_GROUPS', '3')
    monkeypatch.setenv('AVR_ROLLOUT', mode)
    A, md, S16 = feeding
    P, O = feeding_pool
    S = stage(md, np.tile(S16, (5, 1)), D7)
    out, (per_slot, ep, rolls) = check_policy_identity(md, S, P, O, policy25[2], 3, 19)
    assert rolls[31] > 0 and rolls[32] > 0 and rolls[79] > 0
    assert all(rolls[lo:hi].any() for lo, hi in ((0, 32), (32, 64), (64, 80)))
    assert rolls.max() >= 2                                  # (some env rolled twice: episode = 1 was used)
    assert np.all(per_slot[[0, 1, 14, 15, 16, 18]] > 0) and np.all(rolls[6::7] == 0)
    # the finishing step's done marks the boundary; the next slot's observation is a pool observation
    done = out['done'] != 0
    k, e = np.nonzero(done)
    assert all(any(np.array_equal(out['obs'][kk + 1, ee], o) for o in O) for kk, ee in zip(k, e))


@pytest.mark.parametrize('task', ['scratch', 'bedbath'])
def test_rollover_equals_host_loop_pr2(task, monkeypatch):
    """ScratchItchPR2 (obs 30) and BedBathingPR2 (obs 24; the stall kernel rewrites rew after the task
    kernel: the rollover is ordered behind it), 1361 words: the dword copy.  64 envs in 2 groups,
    branches by default."""
    from avr import _abi as ABI, policy_eval as PE
    monkeypatch.setenv('AVR_ENV_GROUPS', '2')
    monkeypatch.delenv('AVR_ROLLOUT', raising=False)
    if task == 'scratch':
        import scratch_util as SU
        A, md = SU.scene()
        S8, _ = SU.reset_states(A, md, range(8))
    else:
        from avr import reset_bedbath as RBB
        A = ABI.load_scene(ABI.TASK_BEDBATH)
        md = ABI.ModelDesc(A)
        S8, _ = RBB.batch_reset_states(A, md, SEED, list(range(8)), attempts=12, iters=80)
    S8 = S8.astype(np.float32)
    od = md.layout.OBS_DIM
    P, O = make_pool(md, S8, (5, 1, 6, 2, 4), 3)
    pol, rms = random_policy(od, 7, 48, seed=5)
    S = stage(md, np.tile(S8, (8, 1)), D7)
    out, (per_slot, ep, rolls) = check_policy_identity(md, S, P, O, PE.policy_desc(pol, rms, od, 7), 2, 19)
    assert rolls[31] > 0 and rolls[32] > 0 and rolls.max() >= 2 and per_slot.sum() == rolls.sum()
    assert np.all(np.isfinite(out['rew'][out['done'] != 0]))     # (the finishing steps' rewards, equal to the loop's above)


def _random_buffers(n, K, od):
    import torch
    from avr import _abi as ABI
    z = lambda *s, **kw: torch.zeros(*s, device='cuda', **kw)
    return dict(obs=z(K, n, od), rew=z(K, n), done=z(K, n, dtype=torch.uint8), info=z(K, n, ABI.INFO_DIM))


def test_random_rollouts(feeding, feeding_pool, monkeypatch):
    """avr_rollout_random_device with the mode on, stacked and non-stacked, 19 steps == the loop of
    avr_step_random_device, avr_rollover_device and sync; the non-stacked run leaves the reset
    observation of the envs the last step finished in the caller's buffer."""
    import torch
    monkeypatch.setenv('AVR_ENV_GROUPS', '3')
    monkeypatch.delenv('AVR_ROLLOUT', raising=False)
    A, md, S16 = feeding
    P, O = feeding_pool
    n, K, t0 = 80, 19, 3
    S = stage(md, np.tile(S16, (5, 1)), D7)
    per_slot, ep_plan, rolls = plan(md, S, P, K)
    assert per_slot[K - 1] > 0
    a, b = make_sim(md, n), make_sim(md, n)
    for s in (a, b):
        s.set_state(S)
        s.reset_pool_set(P, O)
    a.rollover_enable(True)
    Ba, Bb, Bc = _random_buffers(n, K, 25), _random_buffers(n, K, 25), _random_buffers(n, 1, 25)
    torch.cuda.synchronize()
    c0 = a.graph_captures()
    a.rollout_random_device(t0, K, *(Ba[k].data_ptr() for k in ('obs', 'rew', 'done', 'info')), stacked=True)
    a.sync()
    assert a.graph_captures() == c0 + 1
    Sa, ra = a.get_state(), rollover_rows(a)
    a.set_state(S)                      # the same rollout again, non-stacked, from the same state and counters
    a.rollover_set_episodes(np.zeros(n, np.int32))
    a.rollout_random_device(t0, K, *(Bc[k].data_ptr() for k in ('obs', 'rew', 'done', 'info')), stacked=False)
    a.sync()
    assert a.graph_captures() == c0 + 2
    T = _random_buffers(n, 1, 25)       # (one set of step buffers: the reference loop captures one step graph)
    torch.cuda.synchronize()
    for k in range(K):          # (the handle's rollover mode is off: the per-step calls)
        b.step_random_device(t0 + k, *(T[q].data_ptr() for q in ('obs', 'rew', 'done', 'info')))
        b.rollover_device(T['done'].data_ptr(), T['obs'].data_ptr())
        b.sync()
        for q in T:
            Bb[q][k].copy_(T[q][0])
        torch.cuda.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(Bb['done'].cpu().numpy().sum(1), per_slot)
    Sb = b.get_state()
    assert np.array_equal(Sa, Sb) and np.array_equal(a.get_state(), Sb)
    for k in Ba:
        assert torch.equal(Ba[k], Bb[k]), k
        assert torch.equal(Bc[k][0], Bb[k][K - 1]), k
    rb = rollover_rows(b)
    for rs in (ra, rollover_rows(a)):
        assert np.array_equal(rs[0], rb[0]) and np.array_equal(rs[2], rb[2]) and np.array_equal(rs[2], ep_plan)
    last = np.nonzero(Bb['done'][K - 1].cpu().numpy())[0]
    lo = Bc['obs'][0].cpu().numpy()[last]
    assert len(last) and all(any(np.array_equal(row, o) for o in O) for row in lo)
    a.close()
    b.close()


def test_mode_off_is_untouched(feeding, feeding_pool, monkeypatch):
    """A pool installed but the mode off: a rollout across a boundary equals that of a handle that never
    saw a pool (done stays set, T_ITER runs past max_steps); toggling on / off / on re-uses both graphs."""
    import torch
    monkeypatch.setenv('AVR_ENV_GROUPS', '3')
    monkeypatch.delenv('AVR_ROLLOUT', raising=False)
    A, md, S16 = feeding
    P, O = feeding_pool
    L, ms = md.layout, int(md.params['max_episode_steps'])
    n, K = 80, 19
    S = stage(md, np.tile(S16, (5, 1)), D7)
    p, q = make_sim(md, n), make_sim(md, n)
    p.reset_pool_set(P, O)
    Bp, Bq = _random_buffers(n, K, 25), _random_buffers(n, K, 25)
    torch.cuda.synchronize()
    for s, B in ((p, Bp), (q, Bq)):
        s.set_state(S)
        s.rollout_random_device(0, K, *(B[k].data_ptr() for k in ('obs', 'rew', 'done', 'info')), stacked=True)
        s.sync()
    Sp = p.get_state()
    assert np.array_equal(Sp, q.get_state())
    for k in Bp:
        assert torch.equal(Bp[k], Bq[k]), k
    done = Bp['done'].cpu().numpy()
    for e in range(n):
        d = D7[e % 7]
        assert np.array_equal(done[:, e] != 0, np.arange(K) >= d - 1 if d else np.zeros(K, bool))
    assert np.array_equal(Sp[:, L.S_TASK + L.T_ITER], S[:, L.S_TASK + L.T_ITER] + K) and Sp[:, L.S_TASK + L.T_ITER].max() > ms
    assert np.all(rollover_rows(p)[2] == 0)
    c = p.graph_captures()
    for on, new in ((True, 1), (False, 0), (True, 0)):
        p.rollover_enable(on)
        p.set_state(S)
        p.rollout_random_device(0, K, *(Bp[k].data_ptr() for k in ('obs', 'rew', 'done', 'info')), stacked=True)
        p.sync()
        c += new
        assert p.graph_captures() == c, (on, new)
        if on:
            assert not torch.equal(Bp['obs'], Bq['obs']) and not torch.equal(Bp['done'], Bq['done'])
        else:
            assert all(torch.equal(Bp[k], Bq[k]) for k in Bp)
    p.close()
    q.close()


def test_pool_replacement_needs_no_recapture(feeding, feeding_obs16, feeding_pool, policy25, monkeypatch):
    """After a rollout, a smaller pool of other rows: the next rollout takes its rows from the new pool
    (the states equal the host loop's) with no new capture."""
    import torch
    monkeypatch.setenv('AVR_ENV_GROUPS', '3')
    monkeypatch.delenv('AVR_ROLLOUT', raising=False)
    A, md, S16 = feeding
    P, O = feeding_pool
    n, K = 80, 5
    D = (1, 2, 4, None)
    S = stage(md, np.tile(S16, (5, 1)), D)
    a, b = make_sim(md, n), make_sim(md, n)
    for s in (a, b):
        s.set_state(S)
        obs0 = s.settle(2)
        s.policy_set(policy25[2])
        s.reset_pool_set(P, O)
    a.rollover_enable(True)
    obs0 = torch.from_numpy(obs0).cuda()
    Ba, Bb = _stacked(n, K, 25), _stacked(n, K, 25)
    torch.cuda.synchronize()
    _rollout(a, 0, K, obs0, False, Ba)
    a.sync()
    c = a.graph_captures()
    P2, O2 = pick_pool(md, S16, feeding_obs16, (14, 0, 8), 1)
    assert not any(np.array_equal(o, o2) for o in O for o2 in O2)
    ep0 = np.arange(n) % 3
    for s in (a, b):
        s.reset_pool_set(P2, O2)
        s.rollover_set_episodes(ep0)
        s.set_state(S)
        s.settle(2)
    assert a.graph_captures() == c
    _rollout(a, 7, K, obs0, False, Ba)
    a.sync()
    assert a.graph_captures() == c
    ep = ep0.astype(np.int64)
    term = loop_policy(b, 7, K, obs0, False, Bb, P2, O2, ep)
    torch.cuda.synchronize()
    assert np.array_equal(a.get_state(), b.get_state())
    for k in Ba:
        assert torch.equal(Ba[k], Bb[k]), k
    to, _, de = rollover_rows(a)
    assert np.array_equal(de, ep) and np.array_equal(to[ep > ep0], term[ep > ep0]) and (ep > ep0).sum() >= n // 2
    with pytest.raises(RuntimeError, match='exceeds the pool block'):
        a.reset_pool_set(np.tile(P, (2, 1)), np.tile(O, (2, 1)))
    a.close()
    b.close()


@pytest.mark.parametrize('env', [{'AVR_ENV_GROUPS': '1'}, {'AVR_ENV_GROUPS': '2', 'AVR_GRAPH': '0'}], ids=['one-group', 'no-graph'])
def test_direct_loop_fallback_rolls_over(feeding, feeding_pool, policy25, monkeypatch, env):
    """One env group, or AVR_GRAPH=0: the rollout's direct loop calls the stand-alone rollover after every
    step; same identity with 64 envs and K = 4."""
    A, md, S16 = feeding
    for k in ('AVR_ENV_GROUPS', 'AVR_GRAPH', 'AVR_ROLLOUT'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    P, O = feeding_pool
    S = stage(md, np.tile(S16, (4, 1)), (1, 2, 4, None))
    _, (per_slot, ep, rolls) = check_policy_identity(md, S, P, O, policy25[2], int(env['AVR_ENV_GROUPS']), 4, graph=False)
    assert per_slot[0] > 0 and per_slot[1] > 0 and per_slot[3] > 0 and rolls.max() >= 2


def test_errors(feeding, feeding_pool):
    import ctypes as C
    import torch
    from avr import _abi as ABI, reset_dressing as RD
    A, md, S16 = feeding
    P, O = feeding_pool
    n = 8
    sim = make_sim(md, n)
    lib, h = sim.lib, sim.h
    dn, ob = torch.zeros(n, dtype=torch.uint8, device='cuda'), torch.zeros(n, 25, device='cuda')
    torch.cuda.synchronize()
    for call in (lambda: sim.rollover_enable(True), lambda: sim.rollover_device(dn.data_ptr(), ob.data_ptr()), sim.rollover_buffers,
                 lambda: sim.rollover_set_episodes(np.zeros(n, np.int32))):
        with pytest.raises(RuntimeError, match='avr_reset_pool_set first'):
            call()
    assert lib.avr_reset_pool_set(h, 0, P.ctypes.data, O.ctypes.data) == -1 and b'n_pool 0' in lib.avr_last_error(h)
    assert lib.avr_reset_pool_set(h, 5, None, O.ctypes.data) == -1 and b'must be given' in lib.avr_last_error(h)
    assert lib.avr_reset_pool_set(h, 5, P.ctypes.data, None) == -1
    with pytest.raises(RuntimeError, match='avr_reset_pool_set first'):       # (none of the rejected ones was installed)
        sim.rollover_enable(True)
    sim.reset_pool_set(P[:3], O[:3])
    with pytest.raises(RuntimeError, match='exceeds the pool block'):
        sim.reset_pool_set(P, O)
    assert lib.avr_rollover_device(h, None, ob.data_ptr()) == -1 and b'must be given' in lib.avr_last_error(h)
    assert lib.avr_rollover_device(h, dn.data_ptr(), None) == -1
    assert lib.avr_rollover_set_episodes(h, None) == -1 and b'NULL' in lib.avr_last_error(h)
    # the handle is still usable: a rollover of env 2 lands
    sim.set_state(S16[:n])
    sim.rollover_enable(True)
    dn[2] = 1
    torch.cuda.synchronize()
    sim.rollover_device(dn.data_ptr(), ob.data_ptr())
    sim.sync()
    from avr import _lib
    j = int(_lib.rollover_index(SEED, [2], [0], 3)[0])
    St = sim.get_state()
    assert np.array_equal(St[2], P[j]) and np.array_equal(np.delete(St, 2, 0), np.delete(S16[:n], 2, 0))
    assert np.array_equal(ob.cpu().numpy()[2], O[j]) and rollover_rows(sim)[2].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    sim.close()
    dr = make_sim(ABI.ModelDesc(RD.dressing_scene()), 2)
    vp = C.c_void_p()
    for rc in (dr.lib.avr_reset_pool_set(dr.h, 1, None, None), dr.lib.avr_rollover_enable(dr.h, 1), dr.lib.avr_rollover_device(dr.h, None, None),
               dr.lib.avr_rollover_buffers(dr.h, C.byref(vp), None, None), dr.lib.avr_rollover_set_episodes(dr.h, None)):
        assert rc == -1 and b'not built for DressingJaco' in dr.lib.avr_last_error(dr.h)
    dr.close()


def test_torch_facade(feeding, policy25):
    """AVRTorchVecEnv(reset_pool=1): no cap on n, no host reset; mirrors, pool observations, terminal
    observations and step()'s terminal_observation; reset_pool=None keeps the cap and the reset mask."""
    import torch
    from avr import _lib
    from avr.env import AVRTorchVecEnv
    A, md, _ = feeding
    pol, rms, d = policy25
    L, ms = md.layout, int(md.params['max_episode_steps'])
    n, K = 32, 24
    env = AVRTorchVecEnv('FeedingJaco-v0', n, reset_pool=1)
    obs0 = env.reset()
    assert env.pool_build_s > 0 and np.all(env.episode == 0) and np.all(env.iteration == 0)
    P, PO = env.get_state(), obs0.cpu().numpy()              # (reset_pool=1: the pool is the envs' reset states)
    # the pool observation is the pool state's own: settle(0) on a second handle reproduces it bit for bit
    sim = make_sim(md, n)
    sim.set_state(P)
    assert np.array_equal(sim.settle(0), PO)
    D = (3, 10, 24, None)
    env.set_state(stage(md, P, D))
    assert env.iteration[0] == ms - 3 and env.iteration[3] == 0
    out = env.rollout_policy(pol, rms, K)
    torch.cuda.synchronize()
    assert out['n'] == K                                     # (no cap at the TimeLimit)
    done = out['done'].cpu().numpy() != 0
    assert torch.equal(out['reset'], out['done'].bool().any(0)) and out['reset'].dtype == torch.bool and out['reset'].is_cuda
    assert np.array_equal(done.any(0), np.array([D[e % 4] is not None for e in range(n)]))
    S1 = env.get_state()
    to, tv, de = rollover_rows(env.sim)
    assert np.array_equal(env.iteration, S1[:, L.S_TASK + L.T_ITER].astype(np.int64)) and np.array_equal(env.episode, de)
    assert np.array_equal(env.iteration, np.array([K - D[e % 4] if D[e % 4] else K for e in range(n)]))
    obs = out['obs'].cpu().numpy()
    for k, e in zip(*np.nonzero(done)):
        assert np.array_equal(obs[k + 1, e], PO[int(_lib.rollover_index(SEED, [e], [0], n)[0])])
    # term_obs / term_value: the host loop's terminal observation and its value
    sim.set_state(stage(md, P, D))
    sim.policy_set(d)
    B = _stacked(n, K, 25)
    term = loop_policy(sim, 0, K, obs0, False, B, P, PO, np.zeros(n, np.int64))
    assert torch.equal(out['obs'], B['obs']) and np.array_equal(out['term_obs'].cpu().numpy(), term)
    assert np.array_equal(out['term_value'].cpu().numpy(), term_values(sim, term)) and np.array_equal(to, term)
    assert np.array_equal(S1, sim.get_state())
    sim.close()
    # step() with a pool: the boundary without a host reset; terminal_observation from the handle's rows
    S2 = S1.copy()
    S2[:, L.S_TASK + L.T_ITER] = np.where(np.arange(n) % 2 == 0, ms - 1, 5)
    env.set_state(S2)
    ep0, rt = env.episode.copy(), env.reset_timing
    o, r, dn, info = env.step(torch.zeros(n, 7, device='cuda'))
    torch.cuda.synchronize()
    dn = dn.cpu().numpy()
    assert env.reset_timing is rt                            # (no host reset ran)
    assert np.array_equal(dn, np.arange(n) % 2 == 0) and np.array_equal(env.episode, ep0 + dn)
    assert np.array_equal(env.iteration, np.where(dn, 0, 6)) and np.array_equal(rollover_rows(env.sim)[2], env.episode)
    j = _lib.rollover_index(SEED, np.nonzero(dn)[0], ep0[dn], n)
    assert np.array_equal(o.cpu().numpy()[dn], PO[j])
    tob = info['terminal_observation'].cpu().numpy()
    assert np.array_equal(tob[~dn], o.cpu().numpy()[~dn]) and not np.array_equal(tob[dn], PO[j])
    assert np.array_equal(tob[dn], rollover_rows(env.sim)[0][dn])
    env.close()
    # reset_pool=None: today's behaviour -- the cap at the TimeLimit, host reset, the reset mask
    env = AVRTorchVecEnv('FeedingJaco-v0', n)
    env.reset()
    S = env.get_state()
    S[:, L.S_TASK + L.T_ITER] = ms - 3
    env.set_state(S)
    out = env.rollout_policy(pol, rms, K)
    assert out['n'] == 3 and 'term_obs' not in out and bool(out['reset'].all()) and np.all(env.iteration == 0) and np.all(env.episode == 1)
    env.close()
