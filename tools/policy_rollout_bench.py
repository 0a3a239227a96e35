#!/usr/bin/env python
"""Policy-in-the-loop step rate, three ways in one process on one GPU (default: FeedingJaco-v0,
4096 envs, 200 steps, stochastic actions, bench.py's synthetic policy):

  eager   avr.policy_eval.evaluate(fused=False): torch normalise + MLP forward, then
          AVRTorchVecEnv.step, per step (what bench.py --policy-eval times);
  fused   avr.policy_eval.evaluate(fused=True): the policy on the device inside the rollout graphs
          (AVRTorchVecEnv.rollout_policy, 50 steps per call);
  random  Sim.rollout_random_device with stacked outputs, 50 steps per call: the ceiling (no policy).

Every leg makes its own env and resets it; the rate is env-steps over the stepping loop's wall
time, synchronised at both ends (evaluate's loop_s).  The fused and random legs capture their
rollout graphs in one untimed chunk and put the state back; the eager leg's single step graph is
captured inside its timed loop, as in evaluate.  --diagnose adds a fourth leg, fused_zero_mean: the
fused leg with the policy's action head zeroed and std = 0.577, so that its actions have the random
leg's mean and variance -- the policy's own cost, apart from what its actions do to the physics
(a random-init policy's mean drives the arm one way all episode long, into ever more contacts, and
the steps get slower; both policy legs pay that, the random leg does not).  The legs alternate
over --rounds rounds so that drift of the shared host shows as spread, not as a difference;
medians and every sample are written to --out (default profiles/policy_rollout.json) and printed
as one JSON line.
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


def random_leg(name, E, steps, chunk):
    """The ceiling: device-random actions, stacked outputs, `chunk` steps per call."""
    import torch
    from avr import _abi as ABI
    from avr.env import AVRTorchVecEnv
    env = AVRTorchVecEnv(name, E, auto_reset=False)
    try:
        env.reset()
        L, dev = env.L, env.dev
        bufs = (torch.zeros(chunk, E, L.OBS_DIM, device=dev), torch.zeros(chunk, E, device=dev),
                torch.zeros(chunk, E, dtype=torch.uint8, device=dev), torch.zeros(chunk, E, ABI.INFO_DIM, device=dev))
        ptr = [b.data_ptr() for b in bufs]
        ret = torch.zeros(E, device=dev)
        S = env.get_state()
        torch.cuda.synchronize(dev)
        env.sim.rollout_random_device(0, chunk, *ptr, stacked=True)       # untimed: captures the graphs
        env.sim.sync()
        env.set_state(S)
        t0 = time.perf_counter()
        for k in range(0, steps, chunk):
            n = min(chunk, steps - k)
            env.ext.wait_stream(torch.cuda.current_stream(dev))
            env.sim.rollout_random_device(k, n, *ptr, stacked=True)
            torch.cuda.current_stream(dev).wait_stream(env.ext)
            ret += bufs[1][:n].sum(0)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0
    finally:
        env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--task', default='FeedingJaco-v0')
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--diagnose', action='store_true', help='add the fused_zero_mean leg (see above)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'policy_rollout.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('policy_rollout_bench: no GPU (the rates are measured on the device or not at all)')
    from avr import policy_eval as PE
    from avr.env import REGISTRY, _TASK_OF
    from avr import _abi as ABI
    L = ABI.LAYOUTS[_TASK_OF[REGISTRY[args.task][0]]]
    torch.manual_seed(0)
    pol = PE.ActorCritic(L.OBS_DIM, L.ACT_DIM)
    rms = PE.RunningMeanStd((L.OBS_DIM,))
    E, steps = args.envs, args.steps
    legs = {
        'eager': lambda: PE.evaluate(args.task, pol, rms, n_envs=E, steps=steps, deterministic=False)['loop_s'],
        'fused': lambda: PE.evaluate(args.task, pol, rms, n_envs=E, steps=steps, deterministic=False, fused=True)['loop_s'],
        'random': lambda: random_leg(args.task, E, steps, PE.FUSED_CHUNK),
    }
    if args.diagnose:
        zero = PE.ActorCritic(L.OBS_DIM, L.ACT_DIM)
        with torch.no_grad():
            zero.mu.weight.zero_()
            zero.mu.bias.zero_()
            zero.logstd.fill_(-0.5493)            # std 0.577 = the standard deviation of U(-1, 1)
        legs['fused_zero_mean'] = lambda: PE.evaluate(args.task, zero, rms, n_envs=E, steps=steps, deterministic=False, fused=True)['loop_s']
    rates = {k: [] for k in legs}
    for r in range(args.rounds):
        for k, f in legs.items():
            s = f()
            rates[k].append(E * steps / s)
            print('round %d %-15s %8.2f ms/step %10.0f env-steps/s' % (r, k, s / steps * 1e3, rates[k][-1]), file=sys.stderr, flush=True)
    med = {k: statistics.median(v) for k, v in rates.items()}
    out = {'metric': 'policy-in-the-loop env-steps/s of the stepping loop, three legs alternated in one process (medians)',
           'unit': 'env-steps/s', 'task': args.task, 'envs': E, 'steps': steps, 'rounds': args.rounds, 'stochastic': True,
           'fused_chunk': PE.FUSED_CHUNK, 'eager': med['eager'], 'fused': med['fused'], 'random_rollout': med['random'],
           'fused_over_eager': med['fused'] / med['eager'], 'fused_over_random': med['fused'] / med['random'],
           'samples': rates, 'device': torch.cuda.get_device_name(0)}
    if args.diagnose:
        out['fused_zero_mean'] = med['fused_zero_mean']
        out['fused_zero_mean_over_random'] = med['fused_zero_mean'] / med['random']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
