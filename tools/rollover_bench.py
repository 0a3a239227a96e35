#!/usr/bin/env python
"""What the device-side episode rollover (include/avr.h avr_rollover_*) costs and what it buys, in
one process on one GPU (FeedingJaco-v0, 4096 envs), written to profiles/rollover.json:

  (a) overhead   a 192-step random stacked rollout from a fresh reset (no env finishes), with the
                 rollover mode off and on, interleaved over --repeats repeats: mode on replaces the
                 stacked step's slot-copy launch by the rollover-and-copy launch and adds none, so the
                 two should not differ by more than the repeats' spread.  --parent-lib PATH adds the
                 mode-off figure of another build of libavr.so (the parent commit's), measured by a
                 child process of this tool under its own time limit.
  (b) trainer    600 policy steps (three episodes) through AVRTorchVecEnv.rollout_policy in 128-step
                 rollouts, with reset_pool=None (n capped at the TimeLimit, a synchronisation and the
                 host reset at each boundary) and with reset_pool=1 (no cap, no host work); the
                 pool's construction is timed separately.  One untimed pass each captures the graphs.

Rates are env-steps over wall time, synchronised at both ends; medians, every sample and the spread
(max - min over the median) are reported, and printed as one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
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


def overhead(E, steps, repeats, modes):
    """(a): env-steps/s of a `steps`-step random stacked rollout per rollover mode, interleaved."""
    import torch
    from avr import _abi as ABI
    from avr.env import AVRTorchVecEnv
    env = AVRTorchVecEnv(TASK, E, auto_reset=False)
    try:
        obs0 = env.reset()
        L, dev, sim = env.L, env.dev, env.sim
        S = env.get_state()
        if True in modes:
            sim.reset_pool_set(S, obs0.cpu().numpy())
        bufs = (torch.zeros(steps, E, L.OBS_DIM, device=dev), torch.zeros(steps, E, device=dev),
                torch.zeros(steps, E, dtype=torch.uint8, device=dev), torch.zeros(steps, E, ABI.INFO_DIM, device=dev))
        ptr = [b.data_ptr() for b in bufs]

        def run(on):
            if True in modes:
                sim.rollover_enable(on)
            env.set_state(S)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            sim.rollout_random_device(0, steps, *ptr, stacked=True)
            sim.sync()
            dt = time.perf_counter() - t0
            assert not bool(bufs[2].any())              # (no env finished: the rollover itself never ran)
            return E * steps / dt
        for on in modes:                                # untimed: captures each mode's graphs
            run(on)
        rates = {on: [] for on in modes}
        for r in range(repeats):
            for on in modes:
                rates[on].append(run(on))
                print('(a) repeat %d mode %-3s %10.0f env-steps/s' % (r, 'on' if on else 'off', rates[on][-1]), file=sys.stderr, flush=True)
        return rates
    finally:
        env.close()


def trainer(E, total, chunk, repeats, reset_pool):
    """(b): env-steps/s of `total` policy steps in `chunk`-step rollout_policy calls."""
    import torch
    from avr import policy_eval as PE
    from avr.env import AVRTorchVecEnv
    torch.manual_seed(0)
    env = AVRTorchVecEnv(TASK, E, reset_pool=reset_pool)
    L = env.L
    pol, rms = PE.ActorCritic(L.OBS_DIM, L.ACT_DIM), PE.RunningMeanStd((L.OBS_DIM,))
    try:
        env.set_policy(pol, rms)
        rates, calls = [], []
        for r in range(repeats + 1):                    # (pass 0 untimed: buffers and graphs)
            env.reset()
            torch.cuda.synchronize(env.dev)
            t0, done, n_calls = time.perf_counter(), 0, 0
            while done < total:
                done += env.rollout_policy(None, None, min(chunk, total - done))['n']
                n_calls += 1
            torch.cuda.synchronize(env.dev)
            dt = time.perf_counter() - t0
            if r:
                rates.append(E * total / dt)
                calls.append(n_calls)
                print('(b) repeat %d reset_pool=%s %10.0f env-steps/s in %d calls' % (r - 1, reset_pool, rates[-1], n_calls), file=sys.stderr, flush=True)
        return rates, calls[0], env.pool_build_s
    finally:
        env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=192, help='(a): steps of the random rollout')
    ap.add_argument('--repeats', type=int, default=5, help='(a): repeats per mode (at least 5)')
    ap.add_argument('--policy-steps', type=int, default=600, help='(b): policy steps per pass')
    ap.add_argument('--chunk', type=int, default=128, help='(b): steps per rollout_policy call')
    ap.add_argument('--repeats-b', type=int, default=3, help='(b): timed passes per setting')
    ap.add_argument('--parent-lib', default=None, help="(a): another build's libavr.so for the mode-off reference")
    ap.add_argument('--parent-timeout', type=int, default=240, help='time limit (s) of the --parent-lib child process')
    ap.add_argument('--only-off', action='store_true', help='(internal) print the mode-off rates of (a) as JSON and exit')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rollover.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('rollover_bench: no GPU (the rates are measured on the device or not at all)')
    E = args.envs
    if args.only_off:
        print(json.dumps(overhead(E, args.steps, args.repeats, (False,))[False]), flush=True)
        return
    rates = overhead(E, args.steps, args.repeats, (False, True))
    off, on = summary(rates[False]), summary(rates[True])
    a = {'steps': args.steps, 'repeats': args.repeats, 'mode_off': off, 'mode_on': on, 'on_over_off': on['median'] / off['median'],
         'within_spread': abs(on['median'] / off['median'] - 1.0) <= max(off['spread'], on['spread'])}
    if args.parent_lib:
        # a fresh child process (its own HIP runtime and library) under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), '--only-off', '--envs', str(E), '--steps', str(args.steps), '--repeats', str(args.repeats)]
        r = subprocess.run(cmd, env=dict(os.environ, AVR_LIB=os.path.abspath(args.parent_lib)), stdout=subprocess.PIPE, timeout=args.parent_timeout, check=True)
        a['parent_mode_off'] = summary(json.loads(r.stdout.decode().strip().splitlines()[-1]))
        a['off_over_parent'] = off['median'] / a['parent_mode_off']['median']
    host, host_calls, _ = trainer(E, args.policy_steps, args.chunk, args.repeats_b, None)
    pool, pool_calls, build_s = trainer(E, args.policy_steps, args.chunk, args.repeats_b, 1)
    hs, ps = summary(host), summary(pool)
    b = {'policy_steps': args.policy_steps, 'chunk': args.chunk, 'repeats': args.repeats_b, 'reset_pool_none': dict(hs, calls=host_calls),
         'reset_pool_1': dict(ps, calls=pool_calls), 'pool_build_s': build_s, 'pool_over_none': ps['median'] / hs['median']}
    out = {'metric': 'device-side episode rollover: (a) random stacked rollout, mode off vs on; (b) rollout_policy across episode boundaries',
           'unit': 'env-steps/s', 'task': TASK, 'envs': E, 'overhead': a, 'trainer': b, 'device': torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
