#!/usr/bin/env python
"""What the PPO update in segments (include/avr.h avr_ppo_grad_segment_device / avr_ppo_combine_device)
costs next to the single-call update, on one GPU with synthetic batches (a FeedingJaco handle of 8 envs
holds the weights; the batches are random tensors of a rollout's shapes), written to
profiles/dist_ppo.json.  Each figure is the time of 4 epochs x 8 minibatches with permutations drawn
beforehand:

  (i)   avr_ppo_update_device on 128 x 4096 samples: the one-GPU update as it is.
  (ii)  the same call on 128 x 32768 samples: what every rank would pay if 8 ranks each ran the whole
        update on the gathered batch.
  (iii) 128 x 32768 samples, per minibatch one segment + combine + Adam (after one
        avr_ppo_advstat_device): one rank's share at 8 ranks.
  (iv)  128 x 4096 samples, per minibatch all eight segments + combine + Adam: the segmented path run
        by one process, against (i).

The all-gather of the segment rows between the ranks (8 rows of about 52 KB per minibatch) is not part
of any figure: it needs more than one GPU.  Times are wall times synchronised at both ends; the four
are measured in turn within each repeat (interleaved); medians, every sample and the spread (max - min
over the median) are reported, and the result is printed as one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'assistive-vr-gym_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def summary(x):
    med = statistics.median(x)
    return dict(median=med, min=min(x), max=max(x), spread=(max(x) - min(x)) / med, samples=x)


def synthetic_batch(sim, n, E, epochs, seed):
    """(avr_ppo_batch, permutations [epochs, N] int32, the tensors kept alive) of random values with a
    rollout's shapes and magnitudes."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    N = n * E
    r = lambda *s: torch.randn(*s, device='cuda', generator=g)
    T = dict(obs=r(N, sim.obs_dim), act=0.5 * r(N, sim.act_dim), logp=-7.0 + 0.5 * r(N), value=r(N), adv=r(N), ret=r(N))
    perm = torch.stack([torch.randperm(N, device='cuda', generator=g) for _ in range(epochs)]).to(torch.int32).contiguous()
    return sim.ppo_batch(n, E, **{k: v.data_ptr() for k, v in T.items()}), perm, T


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', type=int, default=4096, help='envs of one rank')
    ap.add_argument('--world', type=int, default=8, help='ranks of (ii) and (iii) (divides 8)')
    ap.add_argument('--steps', type=int, default=128, help='steps per rollout')
    ap.add_argument('--repeats', type=int, default=7, help='repeats per measurement (at least 5)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dist_ppo.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('dist_ppo_bench: no GPU (the figures are measured on the device or not at all)')
    from avr import _abi as ABI, _lib, policy_eval as PE, ppo
    E, W, n, R = args.envs, args.world, args.steps, max(args.repeats, 5)
    mine = ppo.segments_of(0, W)
    h = dict(ppo.DEFAULTS)
    epochs, M = h['epochs'], h['n_minibatch']
    torch.manual_seed(0)
    sim = _lib.Sim(ABI.ModelDesc(ABI.load_scene(ABI.TASK_FEEDING)), 8)
    try:
        desc = PE.policy_desc(PE.ActorCritic(sim.obs_dim, sim.act_dim), PE.RunningMeanStd((sim.obs_dim,)), sim.obs_dim, sim.act_dim)
        P = sim.ppo_params(h)
        small = synthetic_batch(sim, n, E, epochs, 1)
        large = synthetic_batch(sim, n, W * E, epochs, 2)
        rows = torch.zeros(_lib.PPO_SEGMENTS, _lib.PPO_SEG_WORDS, device='cuda')
        torch.cuda.synchronize()

        def update(b):
            sim.ppo_update_device(b[0], P, epochs, M, b[1].data_ptr())

        def segmented(b, segments):
            sim.ppo_advstat_device(b[0])
            for ep in range(epochs):
                for j in range(M):
                    for k in segments:
                        sim.ppo_grad_segment_device(b[0], P, j, M, b[1][ep].data_ptr(), k, rows[k].data_ptr())
                    sim.ppo_combine_device(P, rows.data_ptr())
                    sim.ppo_adam_device(P)

        runs = dict(i=lambda: update(small), ii=lambda: update(large), iii=lambda: segmented(large, mine), iv=lambda: segmented(small, range(_lib.PPO_SEGMENTS)))

        def timed(fn):
            sim.policy_set(desc)                               # every run starts from the same weights and zero moments (untimed)
            sim.ppo_reset()
            sim.sync()
            t0 = time.perf_counter()
            fn()
            sim.sync()
            return time.perf_counter() - t0

        for fn in runs.values():                               # untimed warm-ups (code objects)
            timed(fn)
        t = {k: [] for k in runs}
        for r in range(R):
            for k, fn in runs.items():
                t[k].append(timed(fn))
            print('repeat %d: ' % r + ', '.join('(%s) %.2f ms' % (k, 1e3 * t[k][-1]) for k in runs), file=sys.stderr, flush=True)
    finally:
        sim.close()
    S = {k: summary(v) for k, v in t.items()}
    ratio = lambda a, b: dict(median=S[a]['median'] / S[b]['median'], spread=max(S[a]['spread'], S[b]['spread']),
                              per_repeat=summary([x / y for x, y in zip(t[a], t[b])]))
    out = {'metric': 'PPO update in segments, seconds per %d epochs x %d minibatches: (i) update 128 x E, (ii) update 128 x world * E, '
                     '(iii) one rank\'s share of (ii) in segments, (iv) all eight segments on 128 x E' % (epochs, M),
           'envs': E, 'world': W, 'steps': n, 'repeats': R, 'samples': {'i': n * E, 'ii': n * W * E, 'iii': n * W * E, 'iv': n * E},
           'segments_per_minibatch': {'iii': len(mine), 'iv': _lib.PPO_SEGMENTS},
           'seconds': S, 'ii_over_iii': ratio('ii', 'iii'), 'iv_over_i': ratio('iv', 'i'),
           'not_measured': 'the all-gather of the segment rows (8 x %d bytes per minibatch) between ranks: it needs more than one GPU' % (4 * _lib.PPO_SEG_WORDS),
           'device': torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
