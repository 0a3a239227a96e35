"""One rank of the two-rank PPO training test (tests/test_gpu_dist_ppo.py), started by
torch.distributed.run before any process touches the GPU; the test itself imports this module for the
single-process side, so both sides run the same code.

ScratchItchPR2 (no settle frames), E envs per rank on the one GPU the ranks share, gloo.  The envs do
not draw their resets: episode ep of global env g starts from row [ep, g] of an explicit table of host
reset states (state_table), the same rows whatever the rank layout, as gpu_dist_worker.initial_states
does for the rollout test.  AVRTorchVecEnv's own pool building then runs on them, with the all-gather
of the pool rows under test (pool_world).  Each rank writes its weight block, Adam's moments and the
gathered rollouts to <out>.<rank>.npz.  Not a test module.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'assistive-vr-gym_amd'))
sys.path.insert(0, ROOT)

import numpy as np                      # noqa: E402
import torch                            # noqa: E402

POOL_EPISODES = 2
N_STEPS, ITERATIONS = 16, 2
HYPER = dict(epochs=2, n_minibatch=2, lr=1e-3, ent_coef=0.01)
ROLLOUT_KEYS = ('obs', 'act', 'logp', 'rew', 'done')


def state_table(n_global, m=POOL_EPISODES):
    """(md, table [m, n_global, state words] float32): m * n_global distinct host resets (few base-pose
    attempts: speed)."""
    from avr import _abi as ABI, reset_scratch as RSS
    A = ABI.load_scene(ABI.TASK_SCRATCH)
    md = ABI.ModelDesc(A)
    S, _ = RSS.batch_reset_states(A, md, 1001, list(range(m * n_global)), attempts=8, iters=60)
    return md, S.astype(np.float32).reshape(m, n_global, -1)


def near_time_limit(env):
    """Move the envs 20 to 24 steps from the TimeLimit, staggered over the global env ids: they finish
    inside the second rollout, take pool rows on the device, and the advantages bootstrap from terminal
    values.  Only the iteration counter of the state rows changes."""
    L = env.L
    S = env.get_state()
    S[:, L.S_TASK + L.T_ITER] = env.max_steps - 20 - (env.env_offset + np.arange(env.n)) % 5
    env.set_state(S)


def make_env(table, rank, world, group, E):
    """An AVRTorchVecEnv of the rank's E envs whose reset path uploads the table's rows."""
    from avr.env import AVRTorchVecEnv

    class TableEnv(AVRTorchVecEnv):
        def _reset_rows(self, mask):
            idx = np.nonzero(mask)[0]
            S = np.zeros((self.n, self.L.STATE_WORDS), np.float32)
            S[idx] = table[self.episode[idx], self.env_offset + idx]
            self.sim.reset(np.asarray(mask).astype(np.uint8), S, 0, self._obs)
            self.iteration[idx] = S[idx, self.L.S_TASK + self.L.T_ITER].astype(np.int64)

    return TableEnv('ScratchItchPR2-v0', E, env_offset=rank * E, reset_pool=len(table), prefetch=False,
                    pool_world=None if group is None else (rank, world, group))


def train(table, rank, world, group, E):
    """ITERATIONS iterations of DistPPOTrainer on the rank's E envs; returns dict(w, m, v: the weight
    block and Adam's moments; obs, act, logp, rew, done: the gathered rollouts [ITERATIONS * N_STEPS,
    world * E, ...]; stats, episodes: the last iteration's rows)."""
    import copy
    from avr import ppo
    from test_gpu_ppo import policy32
    pol, rms = policy32(30, 64, seed=800)
    env = make_env(table, rank, world, group, E)
    try:
        env.reset()
        near_time_limit(env)
        tr = ppo.DistPPOTrainer(env, copy.deepcopy(pol), copy.deepcopy(rms), n_steps=N_STEPS, generator=torch.Generator(device='cuda').manual_seed(11),
                                group=group, **HYPER)
        rolls = {k: [] for k in ROLLOUT_KEYS}
        for _ in range(ITERATIONS):
            r = tr.iterate()
            for k in ROLLOUT_KEYS:
                rolls[k].append(tr.last['gathered'][k].cpu().numpy().copy())
        torch.cuda.synchronize()
        words = env.sim.ppo_words()
        g, m, v, _ = env.sim.ppo_buffers()
        res = {k: env._wrap(p, (words,), '<f4').cpu().numpy().copy() for k, p in (('w', env.sim.policy_block()), ('m', m), ('v', v))}
        res.update({k: np.concatenate(x, 0) for k, x in rolls.items()})
        res['stats'] = r['stats'].cpu().numpy()
        res['episodes'] = r['episodes'].cpu().numpy()
    finally:
        env.close()
    return res


def main():
    import torch.distributed as dist
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--envs', type=int, default=8, help='envs per rank')
    args = ap.parse_args()
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    dist.init_process_group('gloo')
    _, table = state_table(world * args.envs)
    res = train(table, rank, world, dist.group.WORLD, args.envs)
    np.savez('%s.%d.npz' % (args.out, rank), world=np.int32(world), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
