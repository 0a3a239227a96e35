"""GPU, one process: the PPO update in segments (include/avr.h avr_ppo_advstat_device,
avr_ppo_grad_segment_device, avr_ppo_combine_device; csrc/avr_ppo.hip avr_ppo_combine_kernel) on
FeedingJaco (obs 25) and ScratchItchPR2 (obs 30) handles of 8 envs: the combined gradient against
torch float64 autograd on the whole minibatch, a segment row against the existing gradient call, the
combine kernel against its host mirror bit for bit, independence of the order the rows are filled in,
DistPPOTrainer(group=None) against the loop of raw calls, and the error paths.
The procedures and tolerances are those of tests/test_gpu_ppo.py."""
import numpy as np
import pytest

from test_gpu_ppo import PARAMS, block, check_8x, policy32, reference_grads, stats_row, upload, value_bias_floor
from test_ppo_tasks_host import OBS_DIMS, assert_last_rows_under_test, task_batch

pytestmark = pytest.mark.gpu

TASKS = ('feeding', 'scratch')
N_ENVS = 8
TINY = 2.0 ** -120


@pytest.fixture(scope='module')
def handles():
    """handles(task): the module's one 8-env handle of a task, made at first use and closed at the end.
    No test here needs simulator state: each installs its own policy."""
    from avr import _abi as ABI, _lib
    _lib.load()
    scenes = dict(feeding=ABI.TASK_FEEDING, scratch=ABI.TASK_SCRATCH)
    made = {}

    def get(task):
        if task not in made:
            made[task] = _lib.Sim(ABI.ModelDesc(ABI.load_scene(scenes[task])), N_ENVS)
            assert made[task].obs_dim == OBS_DIMS[task]
        return made[task]
    yield get
    for sim in made.values():
        sim.close()


def install(sim, pol, rms):
    from avr import policy_eval as PE
    sim.policy_set(PE.policy_desc(pol, rms, sim.obs_dim, 7))
    sim.ppo_reset()


def seg_rows():
    import torch
    from avr import _lib
    rows = torch.full((_lib.PPO_SEGMENTS, _lib.PPO_SEG_WORDS), float('nan'), device='cuda')
    torch.cuda.synchronize()
    return rows


def fill_rows(sim, pb, P, j, M, dperm, rows, order=range(8)):
    for k in order:
        sim.ppo_grad_segment_device(pb, P, j, M, None if dperm is None else dperm.data_ptr(), k, rows[k].data_ptr())


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1. accuracy of segments + combine
@pytest.mark.parametrize('N', [128, 192], ids=['seg8', 'seg12'])
@pytest.mark.parametrize('task', TASKS)
def test_combined_gradient_matches_float64_autograd(handles, task, N):
    """Minibatch 1 of 2 of a permuted batch, cut into 8 segments of 8 samples (N = 128: one full pass of one
    block each) or of 12 (N = 192: two blocks, the second with a partial pass of 4): the eight rows combined
    into d_grad against torch float64 autograd of ppo_loss_reference on the whole minibatch, every parameter
    tensor within 8 x the error of torch's CPU float32 autograd against the same float64 (c_b3: the larger of
    that and value_bias_floor); exact zeros outside block_live_mask; the statistics row 1e-5 absolute + 1e-5
    relative.  ent_coef = 0.01: the combine call subtracts it, the segment calls do not.
    Observed on an MI355X, the tensor closest to its bound per case (observed / bound): feeding N = 128 a_w1
    4.4e-7 / 1.8e-6, N = 192 logstd 1.4e-7 / 8.0e-7; scratch N = 128 logstd 1.0e-7 / 7.1e-7, N = 192 a_w1 2.1e-7 /
    1.0e-6: at most 0.25 of the bound.  c_b3 (observed / its bound, the floor): 6.3e-9 .. 3.5e-8 / 8.4e-7 .. 8.7e-7."""
    import torch
    from avr import ppo
    sim = handles(task)
    od = sim.obs_dim
    pol, rms = policy32(od, 64, seed=700 + od)
    batch = task_batch(pol, rms, N, seed=701)
    M, j = 2, 1
    B = N // M
    perm = np.random.default_rng(702).permutation(N).astype(np.int32)
    idx = perm[j * B:(j + 1) * B].astype(np.int64)
    r64, s64 = reference_grads(pol, rms, batch, idx, PARAMS, torch.float64)
    t32, _ = reference_grads(pol, rms, batch, idx, PARAMS, torch.float32)
    assert_last_rows_under_test(r64, batch, idx, rms, od)
    install(sim, pol, rms)
    pb, keep = upload(sim, batch)
    dperm = torch.from_numpy(perm).cuda()
    rows = seg_rows()
    P = sim.ppo_params(PARAMS)
    sim.ppo_advstat_device(pb)
    fill_rows(sim, pb, P, j, M, dperm, rows)
    sim.ppo_combine_device(P, rows.data_ptr())
    g = block(sim, 'g')
    st = stats_row(sim, 0)                    # (the first combine since avr_ppo_advstat_device)
    assert bool(torch.isfinite(rows).all())   # (every word of every row was written)
    assert np.all(g[~ppo.block_live_mask(od, 7, 64)] == 0)
    what = 'segments[%s N=%d]' % (task, N)
    check_8x(what, ppo.unpack_block(g, od, 7, 64), t32, r64, floor=dict(c_b3=value_bias_floor(pol, rms, batch, idx, PARAMS)))
    for i, k in enumerate(('policy_loss', 'value_loss', 'entropy', 'approx_kl', 'clip_frac')):
        print('stat %s %s: device %.9g reference %.9g' % (what, k, st[i], s64[k]))
        assert abs(st[i] - s64[k]) <= 1e-5 + 1e-5 * abs(s64[k]), (k, st[i], s64[k])


# ------------------------------------------------------------------ 2. a segment row against the existing gradient call
@pytest.mark.parametrize('task', TASKS)
def test_segment_row_equals_existing_gradient_call_scaled(handles, task):
    """ent_coef = 0, N = 192, M = 2: segment k of minibatch j is minibatch 8 j + k of 16 for
    avr_ppo_grad_device -- the same 12 samples through the same kernels with the same number of blocks;
    only the weight of a sample differs, 1 / 96 against 1 / 12, a factor of 8 that is exact in every
    product and sum.  So the row's gradient words equal d_grad / 8 and its L_pi, L_v, approx_kl and
    clip_frac words the statistics row's / 8, bit for bit (words below 2^-120 in magnitude on both sides
    count as equal: a division by 8 is not exact among subnormals); the H word is H itself."""
    import torch
    from avr import ppo
    sim = handles(task)
    od = sim.obs_dim
    pol, rms = policy32(od, 64, seed=710 + od)
    N, M = 192, 2
    batch = task_batch(pol, rms, N, seed=711)
    perm = np.random.default_rng(712).permutation(N).astype(np.int32)
    install(sim, pol, rms)
    pb, keep = upload(sim, batch)
    dperm = torch.from_numpy(perm).cuda()
    rows = seg_rows()
    P = sim.ppo_params(dict(PARAMS, ent_coef=0.0))
    sim.ppo_advstat_device(pb)                # (the cache avr_ppo_grad_device reads for minibatches other than 0)
    checked = 0
    for j, k in ((0, 0), (0, 5), (1, 3), (1, 7)):
        sim.ppo_grad_segment_device(pb, P, j, M, dperm.data_ptr(), k, rows[k].data_ptr())
        sim.ppo_grad_device(pb, P, 8 * j + k, 8 * M, dperm.data_ptr())
        g = block(sim, 'g')
        st = stats_row(sim, 8 * j + k)
        row = rows[k].cpu().numpy()
        a, b = row[:ppo.PW_WORDS], g * np.float32(0.125)
        same = (bits(a) == bits(b)) | ((np.abs(a) < TINY) & (np.abs(b) < TINY))
        assert same.all(), (j, k, np.argwhere(~same)[:5].tolist())
        live = ppo.block_live_mask(od, 7, 64)
        assert np.all(a[~live] == 0) and np.count_nonzero(a[live]) > live.sum() // 4      # (a gradient, not zeros)
        tail = row[ppo.PW_WORDS:]
        for t in (0, 1, 3, 4):
            assert bits(tail[t]) == bits(st[t] * np.float32(0.125)) or (abs(tail[t]) < TINY and abs(st[t]) < 8 * TINY), (j, k, t)
        assert bits(tail[2]) == bits(st[2]) and np.all(tail[5:] == 0)
        checked += 1
    assert checked == 4


# ------------------------------------------------------------------ 3. the combine kernel against its mirror
def test_combine_equals_host_mirror_bit_for_bit(handles):
    """Rows of random words of mixed magnitudes, with the order-sensitive word of
    tests/test_ppo_segments_host.py in a weight word and in a statistics word: d_grad equals
    ppo.combine_reference (ascending order, float64, one rounding, ent_coef on the 7 logstd words) on
    every word, the statistics words likewise and H from the weights.  With rows 0 and 2 exchanged the
    crafted words come out one ulp higher on both sides."""
    import torch
    from avr import ppo
    sim = handles('scratch')
    pol, rms = policy32(30, 64, seed=720)
    install(sim, pol, rms)
    rng = np.random.default_rng(721)
    rows = (rng.normal(0, 1, (8, ppo.PPO_SEG_WORDS)) * 10.0 ** rng.integers(-12, 3, (8, ppo.PPO_SEG_WORDS))).astype(np.float32)
    crafted = [1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -24, 0, 0, 0, 0]
    w_word, s_word = ppo.PW_NET + 777, ppo.PW_WORDS + 3
    rows[:, w_word] = crafted
    rows[:, s_word] = crafted
    P = sim.ppo_params(dict(PARAMS, ent_coef=0.25))
    H, w = np.float32(0), block(sim, 'w')
    for a in range(7):                        # (the kernel's float32 sum, in its order)
        H = np.float32(H + np.float32(np.float32(np.float32(0.5) + np.float32(0.9189385332046727)) + w[ppo.PW_LOGSTD + a]))
    pb1, keep1 = upload(sim, dict(adv=np.ones(16, np.float32)))
    for swap, want in ((False, np.float32(1.0)), (True, np.nextafter(np.float32(1.0), np.float32(2.0)))):
        r = rows.copy()
        if swap:
            r[[0, 2]] = r[[2, 0]]
        d = torch.from_numpy(r).cuda()
        torch.cuda.synchronize()
        sim.ppo_advstat_device(pb1)           # (statistics rows restart at 0)
        sim.ppo_combine_device(P, d.data_ptr())
        g, st = block(sim, 'g'), stats_row(sim, 0)
        ref = ppo.combine_reference(r, ent_coef=0.25, act_dim=7)
        assert np.array_equal(bits(g), bits(ref[:ppo.PW_WORDS]))
        assert g[w_word] == want and st[3] == want
        for t in (0, 1, 3, 4):
            assert bits(st[t]) == bits(ref[ppo.PW_WORDS + t]), t
        assert bits(st[2]) == bits(H)
    # the statistics row advances with every combine call and wraps at the ring's length
    sim.ppo_combine_device(P, d.data_ptr())
    assert np.array_equal(bits(stats_row(sim, 1)[:5]), bits(stats_row(sim, 0)[:5]))


# ------------------------------------------------------------------ 4. the order the rows are filled in
def test_rows_filled_in_reverse_order_give_the_same_bits(handles):
    """The eight segment calls in ascending and in descending order (each into its own row), then combine
    and Adam: rows, d_grad, the weight block and both moments are bit-identical -- a segment call leaves
    nothing behind that the next one reads."""
    import torch
    sim = handles('feeding')
    pol, rms = policy32(25, 64, seed=730)
    N, M, j = 192, 2, 1
    batch = task_batch(pol, rms, N, seed=731)
    perm = np.random.default_rng(732).permutation(N).astype(np.int32)
    pb, keep = upload(sim, batch)
    dperm = torch.from_numpy(perm).cuda()
    P = sim.ppo_params(PARAMS)
    outs = []
    for order in (range(8), range(7, -1, -1)):
        install(sim, pol, rms)
        rows = seg_rows()
        sim.ppo_advstat_device(pb)
        fill_rows(sim, pb, P, j, M, dperm, rows, order)
        sim.ppo_combine_device(P, rows.data_ptr())
        sim.ppo_adam_device(P)
        blocks = [block(sim, k) for k in 'gwmv']          # (block() waits for the handle's stream: the rows are complete)
        outs.append([rows.cpu().numpy()] + blocks)
    for a, b in zip(*outs):
        assert np.all(np.isfinite(a)) and np.array_equal(bits(a), bits(b))
    assert np.abs(outs[0][3]).max() > 0       # (Adam ran: first moments)


# ------------------------------------------------------------------ 5. the trainer with group=None is the loop of raw calls
def test_trainer_reference_equals_raw_calls(handles):
    """ScratchItchPR2, 16 envs, reset_pool=1, one DistPPOTrainer(group=None).iterate() of an 8-step rollout
    (N = 128), 2 epochs x 2 minibatches with the running observation statistics on: the weight block, both
    moments and the statistics rows equal, bit for bit, those of a second handle given the same start
    (the policy, then the ob_rms rows the trainer pushed), the trainer's gathered batch and its
    permutations through avr_ppo_advstat_device and the loop of 8 x avr_ppo_grad_segment_device,
    avr_ppo_combine_device, avr_ppo_adam_device."""
    import copy
    import torch
    from avr import _lib, ppo
    from avr.env import AVRTorchVecEnv
    pol, rms = policy32(30, 64, seed=740)
    env = AVRTorchVecEnv('ScratchItchPR2-v0', 16, reset_pool=1)
    env.reset()
    hyper = dict(epochs=2, n_minibatch=2, lr=1e-3, ent_coef=0.01)
    tr = ppo.DistPPOTrainer(env, copy.deepcopy(pol), copy.deepcopy(rms), n_steps=8, generator=torch.Generator(device='cuda').manual_seed(9), **hyper)
    assert tr.segments == list(range(8)) and tr.world == 1
    r = tr.iterate()
    torch.cuda.synchronize()
    got = [block(env.sim, k) for k in 'wmv']
    G, perm = tr.last['gathered'], tr.last['perm']
    out = tr.last['out']
    assert G['obs'].shape == (8, 16, 30) and perm.shape == (2, 128) and r['stats'].shape == (4, 6)
    for k in ('obs', 'value'):                # (the gathered batch of one process is its own rollout)
        assert torch.equal(G[k], out[k][:8])
    assert torch.equal(G['act'], out['act']) and torch.equal(G['adv'], tr.last['adv']) and torch.equal(G['done'], out['done'])
    assert float(r['mean_reward']) == float(out['rew'].mean()) and r['episodes'].shape == (len(_lib.EPISODE_STATS),)
    sim = handles('scratch')
    install(sim, pol, rms)
    sim.policy_obs_norm_device(tr._m32.data_ptr(), tr._v32.data_ptr())
    pb = sim.ppo_batch(8, 16, **{k: G[k].data_ptr() for k in ('obs', 'act', 'logp', 'value', 'adv', 'ret')})
    P = sim.ppo_params(tr.hyper)
    rows = seg_rows()
    sim.ppo_advstat_device(pb)
    for ep in range(2):
        for j in range(2):
            fill_rows(sim, pb, P, j, 2, perm[ep], rows)
            sim.ppo_combine_device(P, rows.data_ptr())
            sim.ppo_adam_device(P)
    want = [block(sim, k) for k in 'wmv']
    st = np.stack([stats_row(sim, i) for i in range(4)])[:, :6]
    stats = r['stats'].cpu().numpy()
    env.close()
    for name, a, b in zip('wmv', got, want):
        assert np.all(np.isfinite(a)) and np.array_equal(bits(a), bits(b)), name
    assert np.array_equal(bits(stats), bits(st)) and np.all(stats[:, 5] > 0)
    # (Adam ran, and the running observation statistics reached the block)
    assert np.abs(got[1]).max() > 0 and not np.array_equal(got[0][ppo.PW_MEAN:ppo.PW_MEAN + 30], rms.mean.astype(np.float32))


# ------------------------------------------------------------------ 6. error paths
def test_errors():
    import ctypes as C
    from avr import _abi as ABI, policy_eval as PE, reset_dressing as RD
    from test_gpu_ppo import make_sim
    A = ABI.load_scene(ABI.TASK_SCRATCH)
    sim = make_sim(ABI.ModelDesc(A), 8)       # (a handle of its own: the first calls come before avr_ppo_reset)
    pol, rms = policy32(30, 64, seed=750)
    batch = task_batch(pol, rms, 128, seed=751)
    pb, keep = upload(sim, batch)
    P = sim.ppo_params(PARAMS)
    rows = seg_rows()
    seg = lambda b=pb, p=P, j=0, M=2, k=0, row=rows[0].data_ptr(): sim.ppo_grad_segment_device(b, p, j, M, None, k, row)
    with pytest.raises(RuntimeError, match='avr_policy_set first'):
        seg()
    with pytest.raises(RuntimeError, match='avr_ppo_reset first'):
        sim.ppo_advstat_device(pb)
    sim.policy_set(PE.policy_desc(pol, rms, 30, 7))
    for call in (seg, lambda: sim.ppo_combine_device(P, rows.data_ptr()), lambda: sim.ppo_advstat_device(pb)):
        with pytest.raises(RuntimeError, match='avr_ppo_reset first'):
            call()
    sim.ppo_reset()
    with pytest.raises(RuntimeError, match='norm_adv without the advantage statistics'):       # (none cached yet)
        seg()
    seg(p=sim.ppo_params(dict(PARAMS, norm_adv=False)))                    # (fine without them)
    sim.ppo_advstat_device(pb)
    seg()
    sim.ppo_reset()                                                        # (forgets them)
    with pytest.raises(RuntimeError, match='norm_adv without the advantage statistics'):
        seg()
    sim.ppo_advstat_device(pb)
    for k in (-1, 8):
        with pytest.raises(RuntimeError, match='segment %d outside 0..7' % k):
            seg(k=k)
    with pytest.raises(RuntimeError, match='minibatch 2 outside'):
        seg(j=2)
    with pytest.raises(RuntimeError, match='d_seg is NULL'):
        seg(row=None)
    with pytest.raises(RuntimeError, match='21 samples does not divide into 8 segments'):   # (128 // 6)
        seg(M=6)
    b70 = sim.ppo_batch(1, 70, **{k: keep[k].data_ptr() for k in keep})
    sim.ppo_advstat_device(b70)
    with pytest.raises(RuntimeError, match='70 samples does not divide into 8 segments'):
        seg(b=b70, M=1)
    with pytest.raises(RuntimeError, match='norm_adv without the advantage statistics'):       # (the cache is the 70-sample batch's)
        seg()
    lib, h = sim.lib, sim.h
    assert lib.avr_ppo_advstat_device(h, None) == -1 and b'batch is NULL' in lib.avr_last_error(h)
    assert lib.avr_ppo_grad_segment_device(h, None, C.byref(P), 0, 1, None, 0, rows.data_ptr()) == -1 and b'batch is NULL' in lib.avr_last_error(h)
    assert lib.avr_ppo_grad_segment_device(h, C.byref(pb), None, 0, 1, None, 0, rows.data_ptr()) == -1 and b'params is NULL' in lib.avr_last_error(h)
    assert lib.avr_ppo_combine_device(h, None, rows.data_ptr()) == -1 and b'params is NULL' in lib.avr_last_error(h)
    assert lib.avr_ppo_combine_device(h, C.byref(P), None) == -1 and b'd_segs is NULL' in lib.avr_last_error(h)
    noadv = sim.ppo_batch(1, 128, **{k: keep[k].data_ptr() for k in keep if k != 'adv'})
    with pytest.raises(RuntimeError, match='adv must be given'):
        sim.ppo_advstat_device(noadv)
    sim.close()
    dr = make_sim(ABI.ModelDesc(RD.dressing_scene()), 2)
    for rc in (dr.lib.avr_ppo_advstat_device(dr.h, None), dr.lib.avr_ppo_grad_segment_device(dr.h, None, None, 0, 1, None, 0, None),
               dr.lib.avr_ppo_combine_device(dr.h, None, None)):
        assert rc == -1 and b'not built for DressingJaco' in dr.lib.avr_last_error(dr.h)
    dr.close()
