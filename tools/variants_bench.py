#!/usr/bin/env python
"""What per-env human height variants (include/avr.h avr_human_variants_set) cost in the step, in one
process on one GPU: FeedingJaco-v0, 4096 envs, impairment 'none', a 192-step random stacked rollout
from a fresh reset

  none      a default handle (no variants loaded: every kernel reads the base tables at offset 0)
  variants  the same id with FeedingJacoNew-v0's grid of 42 heights (21 per gender) loaded and one
            drawn per env: per-env table reads replace the shared ones

interleaved over --repeats repeats after one untimed pass each (graph capture).  Rates are env-steps
over wall time, synchronised at both ends; medians, every sample and the spread (max - min over the
median) are reported and printed as one JSON line (--out writes them to a file as well).
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

TASK = 'FeedingJaco-v0'


def summary(rates):
    med = statistics.median(rates)
    return dict(median=med, min=min(rates), max=max(rates), spread=(max(rates) - min(rates)) / med, samples=rates)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=192)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', choices=('none', 'variants'), default=None,
                    help='run one configuration alone (a kernel trace of it: rocprofv3 --kernel-trace --stats -- python tools/variants_bench.py --only ...)')
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('variants_bench: no GPU (the rates are measured on the device or not at all)')
    from avr import _abi as ABI
    from avr import env as EV
    E, steps = args.envs, args.steps
    make = {'none': lambda: EV.AVRTorchVecEnv(TASK, E, auto_reset=False, impairment='none'),
            'variants': lambda: EV.AVRTorchVecEnv(TASK, E, auto_reset=False, impairment='none', human_heights=EV.new_height_grid())}
    envs = {k: f() for k, f in make.items() if args.only in (None, k)}
    try:
        states, bufs = {}, {}
        for k, env in envs.items():
            env.reset()
            states[k] = env.get_state()
            L, dev = env.L, env.dev
            bufs[k] = (torch.zeros(steps, E, L.OBS_DIM, device=dev), torch.zeros(steps, E, device=dev),
                       torch.zeros(steps, E, dtype=torch.uint8, device=dev), torch.zeros(steps, E, ABI.INFO_DIM, device=dev))
        slots = states['variants' if 'variants' in envs else 'none'][:, L.S_TASK + L.T_GENDER].astype(int)

        def run(k):
            env = envs[k]
            env.set_state(states[k])
            torch.cuda.synchronize(env.dev)
            t0 = time.perf_counter()
            env.sim.rollout_random_device(0, steps, *[b.data_ptr() for b in bufs[k]], stacked=True)
            env.sim.sync()
            return E * steps / (time.perf_counter() - t0)
        for k in envs:
            run(k)
        rates = {k: [] for k in envs}
        for r in range(args.repeats):
            for k in envs:
                rates[k].append(run(k))
                print('repeat %d %-8s %10.0f env-steps/s' % (r, k, rates[k][-1]), file=sys.stderr, flush=True)
        bad = {k: int((envs[k].flags() & 0x1f != 0).sum()) for k in envs}
        if args.only:
            out = {'only': args.only, 'envs': E, 'steps': steps, args.only: summary(rates[args.only]), 'faulted_envs': bad}
            print(json.dumps(out), flush=True)
            return
        a, b = summary(rates['none']), summary(rates['variants'])
        out = {'metric': 'FeedingJaco-v0 random stacked rollout: no variants loaded vs 42 height variants, one per env', 'unit': 'env-steps/s',
               'task': TASK, 'envs': E, 'steps': steps, 'repeats': args.repeats, 'impairment': 'none', 'none': a, 'variants': b,
               'variants_over_none': b['median'] / a['median'], 'within_spread': abs(b['median'] / a['median'] - 1.0) <= max(a['spread'], b['spread']),
               'variants_loaded': len(envs['variants'].variants), 'distinct_slots_in_use': int(len(np.unique(slots))),
               'faulted_envs': bad, 'device': torch.cuda.get_device_name(0)}
    finally:
        for env in envs.values():
            env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
