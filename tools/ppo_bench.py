#!/usr/bin/env python
"""What the PPO update on the device (include/avr.h avr_gae_device / avr_ppo_*) costs next to the
rollout it follows, in one process on one GPU (FeedingJaco-v0, 4096 envs, 128-step rollouts,
reset_pool=1), written to profiles/ppo_update.json:

  (a) update     advantage estimation + the trainer's default epochs x minibatches on one fixed
                 batch: the device path (compute_gae + ppo_update) against the same update in eager
                 torch on the same batch (a vectorised GAE loop, avr/ppo.py ppo_loss_reference,
                 clip_grad_norm_, torch.optim.Adam) followed by set_policy; interleaved repeats.
  (b) iteration  env-steps/s of whole iterations each way (rollout, then (a)'s update), interleaved,
                 and the share of an iteration the update takes (median update time / median
                 iteration time).
  (c) rollout    the rollout alone, with no trainer; --parent-lib PATH adds the same figure for
                 another build of libavr.so (the parent commit's), measured by a child process of
                 this tool under its own time limit.

Times are wall times synchronised at both ends; medians, every sample and the spread (max - min
over the median) are reported, and the result is printed as one JSON line.
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


def summary(x):
    med = statistics.median(x)
    return dict(median=med, min=min(x), max=max(x), spread=(max(x) - min(x)) / med, samples=x)


def timed(dev, fn):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def rollout_only(E, n_steps, repeats):
    """(c): env-steps/s of rollout_policy alone (one untimed pass captures the graphs)."""
    import torch
    from avr import policy_eval as PE
    from avr.env import AVRTorchVecEnv
    torch.manual_seed(0)
    env = AVRTorchVecEnv(TASK, E, reset_pool=1)
    try:
        env.reset()
        env.set_policy(PE.ActorCritic(env.L.OBS_DIM, env.L.ACT_DIM), PE.RunningMeanStd((env.L.OBS_DIM,)))
        env.rollout_policy(None, None, n_steps)
        return [E * n_steps / timed(env.dev, lambda: env.rollout_policy(None, None, n_steps)) for _ in range(repeats)]
    finally:
        env.close()


class Eager:
    """The same update in eager torch on the device tensors of a rollout, then set_policy."""

    def __init__(self, env, actor_critic, ob_rms, hyper):
        import copy
        import torch
        self.env, self.h, self.rms = env, hyper, ob_rms
        self.pol = copy.deepcopy(actor_critic).to(env.dev)
        self.opt = torch.optim.Adam(self.pol.parameters(), lr=hyper['lr'], betas=(hyper['beta1'], hyper['beta2']), eps=hyper['eps'])
        self.drms = type('R', (), dict(mean=torch.as_tensor(ob_rms.mean, dtype=torch.float32, device=env.dev),
                                       var=torch.as_tensor(ob_rms.var, dtype=torch.float32, device=env.dev)))

    def update(self, out):
        import torch
        from avr import ppo
        h = self.h
        n, E = out['rew'].shape
        done, value, rew, tv = out['done'].bool(), out['value'], out['rew'], out['term_value']
        adv = torch.zeros_like(rew)
        gae = torch.zeros(E, device=rew.device)
        for k in range(n - 1, -1, -1):
            nv = torch.where(done[k], tv, value[k + 1])
            gae = (rew[k] + h['gamma'] * nv) - value[k] + h['gamma'] * h['lam'] * torch.where(done[k], torch.zeros_like(gae), gae)
            adv[k] = gae
        batch = ppo.flatten_rollout(out, adv, adv + value[:n])
        N = n * E
        B = N // h['n_minibatch']
        for _ in range(h['epochs']):
            perm = torch.randperm(N, device=rew.device)
            for j in range(h['n_minibatch']):
                self.opt.zero_grad()
                loss, _ = ppo.ppo_loss_reference(self.pol, self.drms, batch, perm[j * B:(j + 1) * B], h)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(self.pol.parameters(), h['max_grad_norm'])
                self.opt.step()
        self.env.set_policy(self.pol, self.rms)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=128, help='steps per rollout')
    ap.add_argument('--repeats', type=int, default=5, help='repeats per measurement (at least 5)')
    ap.add_argument('--parent-lib', default=None, help="(c): another build's libavr.so for the rollout-alone reference")
    ap.add_argument('--parent-timeout', type=int, default=240, help='time limit (s) of the --parent-lib child process')
    ap.add_argument('--only-rollout', action='store_true', help='(internal) print the rates of (c) as JSON and exit')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ppo_update.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('ppo_bench: no GPU (the figures are measured on the device or not at all)')
    E, n, R = args.envs, args.steps, args.repeats
    if args.only_rollout:
        print(json.dumps(rollout_only(E, n, R)), flush=True)
        return
    from avr import policy_eval as PE, ppo
    from avr.env import AVRTorchVecEnv
    c = {'this_tree': summary(rollout_only(E, n, R))}
    if args.parent_lib:
        # a fresh child process (its own HIP runtime and library) under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), '--only-rollout', '--envs', str(E), '--steps', str(n), '--repeats', str(R)]
        r = subprocess.run(cmd, env=dict(os.environ, AVR_LIB=os.path.abspath(args.parent_lib)), stdout=subprocess.PIPE, timeout=args.parent_timeout, check=True)
        c['parent'] = summary(json.loads(r.stdout.decode().strip().splitlines()[-1]))
        c['this_over_parent'] = c['this_tree']['median'] / c['parent']['median']
        c['within_spread'] = abs(c['this_over_parent'] - 1.0) <= max(c['this_tree']['spread'], c['parent']['spread'])
    torch.manual_seed(0)
    env = AVRTorchVecEnv(TASK, E, reset_pool=1)
    try:
        env.reset()
        pol, rms = PE.ActorCritic(env.L.OBS_DIM, env.L.ACT_DIM), PE.RunningMeanStd((env.L.OBS_DIM,))
        tr = ppo.PPOTrainer(env, pol, rms, n_steps=n, update_ob_rms=False)
        h, dev = tr.hyper, env.dev
        eager = Eager(env, pol, rms, h)
        out = env.rollout_policy(None, None, n)               # the fixed batch of (a); untimed: captures the graphs

        def device_update(o):
            adv, ret = env.compute_gae(o, h['gamma'], h['lam'], h['bootstrap'])
            env.ppo_update(o, adv, ret, h, h['epochs'], h['n_minibatch'])

        def device_gae(o):
            env.compute_gae(o, h['gamma'], h['lam'], h['bootstrap'])

        device_update(out)                                    # untimed warm-ups (allocations, code objects, BLAS handles)
        eager.update(out)
        t = dict(device=[], eager=[], device_gae=[])
        for r in range(R):
            t['device'].append(timed(dev, lambda: device_update(out)))
            t['eager'].append(timed(dev, lambda: eager.update(out)))
            t['device_gae'].append(timed(dev, lambda: device_gae(out)))
            print('(a) repeat %d update: device %.2f ms (GAE alone %.3f ms), eager torch + set_policy %.2f ms'
                  % (r, 1e3 * t['device'][-1], 1e3 * t['device_gae'][-1], 1e3 * t['eager'][-1]), file=sys.stderr, flush=True)
        it = dict(device=[], eager=[])
        for r in range(R):
            it['device'].append(timed(dev, lambda: device_update(env.rollout_policy(None, None, n))))
            it['eager'].append(timed(dev, lambda: eager.update(env.rollout_policy(None, None, n))))
            print('(b) repeat %d iteration: device %.1f ms, eager %.1f ms' % (r, 1e3 * it['device'][-1], 1e3 * it['eager'][-1]), file=sys.stderr, flush=True)
    finally:
        env.close()
    a = {k: summary(v) for k, v in t.items()}
    a['eager_over_device'] = a['eager']['median'] / a['device']['median']
    b = {k: dict(seconds=summary(v), env_steps_per_s=summary([E * n / x for x in v])) for k, v in it.items()}
    b['update_share'] = {k: a[k]['median'] / b[k]['seconds']['median'] for k in ('device', 'eager')}
    b['device_over_eager'] = b['device']['env_steps_per_s']['median'] / b['eager']['env_steps_per_s']['median']
    out = {'metric': 'PPO update on the device: (a) update seconds, device vs eager torch + set_policy; (b) whole iterations; (c) rollout alone',
           'task': TASK, 'envs': E, 'steps': n, 'repeats': R, 'samples_per_batch': E * n,
           'hyper': {k: h[k] for k in ('epochs', 'n_minibatch', 'clip', 'vf_coef', 'ent_coef', 'max_grad_norm', 'lr', 'norm_adv', 'clip_value', 'bootstrap')},
           'update': a, 'iteration': b, 'rollout': c, 'device': torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
