"""Multi-GPU plumbing for the vectorised envs.

Envs are independent units: GPU `rank` owns the contiguous block of global env ids
[rank * E, (rank + 1) * E).  Reset randomness and synthetic actions are keyed by the global env
id, so a run's per-env results do not depend on the GPU count.  The only data-path collective is
the rollout collection: each rank packs its (obs, reward, info, done) rows for G steps and one
all_gather_into_tensor (RCCL over xGMI on MI355X; gloo in the CPU tests) concatenates them in
rank order = global env order.  Training across ranks (avr/ppo.py DistPPOTrainer) adds two more
gathers, of the stacked batch and of the minibatch's segment rows (gather_stacked, gather_rows);
it needs no all-reduce either.
"""
import torch

from . import _abi as ABI

ROLL_WIDTH = ABI.OBS_DIM + 1 + ABI.INFO_DIM + 1   # FeedingJaco: obs, reward, info, done


def roll_width(obs_dim):
    """Columns of one env's rollout row: obs, reward, info, done."""
    return obs_dim + 1 + ABI.INFO_DIM + 1


def shard(envs_per_rank, rank):
    """(global id of the rank's first env, count)."""
    return rank * envs_per_rank, envs_per_rank


def pack_rollout(roll, j, obs, rew, info, done):
    """roll[j] (E, W) <- one step of outputs (device tensors, no host sync); W = roll_width(obs_dim)."""
    od = obs.shape[1]
    roll[j, :, :od] = obs
    roll[j, :, od] = rew
    roll[j, :, od + 1:od + 1 + ABI.INFO_DIM] = info
    roll[j, :, -1] = done.to(roll.dtype)


def pack_rollout_stacked(roll, obs, rew, info, done, m):
    """roll[:m] (m, E, W) <- m steps of stacked outputs ([G, E, ...] device tensors); the rows past m
    keep their previous contents (a short last chunk)."""
    od = obs.shape[2]
    roll[:m, :, :od] = obs[:m]
    roll[:m, :, od] = rew[:m]
    roll[:m, :, od + 1:od + 1 + ABI.INFO_DIM] = info[:m]
    roll[:m, :, -1] = done[:m].to(roll.dtype)


def rank_world(group=None):
    """(rank, world size) of a process group (None: the default group)."""
    import torch.distributed as dist
    return dist.get_rank(group), dist.get_world_size(group)


def all_gather_ranks(x, group=None):
    """Every rank's x (same shape and dtype on all ranks) -> [world, *x.shape] in rank order, on x's
    device.  nccl (RCCL) gathers device tensors in place; gloo has no device path, so a device tensor
    is staged through host memory there (the CPU tests, and ranks that share one GPU)."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    x = x.contiguous()
    staged = x.is_cuda and dist.get_backend(group) != 'nccl'
    src = x.cpu() if staged else x
    out = torch.empty((world,) + tuple(src.shape), dtype=src.dtype, device=src.device)
    dist.all_gather_into_tensor(out.reshape(-1), src.reshape(-1), group=group)
    return out.to(x.device) if staged else out


def gather_stacked(x, group=None):
    """Stacked per-rank arrays [n, E, ...] -> [n, world * E, ...] in global env order (rank r owns the
    global env ids [r * E, (r + 1) * E)); a new contiguous tensor on x's device."""
    g = all_gather_ranks(x, group)                          # [world, n, E, ...]
    return g.movedim(0, 1).reshape((x.shape[0], g.shape[0] * x.shape[1]) + tuple(x.shape[2:])).contiguous()


def gather_rows(x, group=None):
    """Small per-rank rows [r, ...] -> [world * r, ...], rank 0's rows first."""
    g = all_gather_ranks(x, group)
    return g.reshape((g.shape[0] * x.shape[0],) + tuple(x.shape[1:]))


def gather_rollouts(roll, out=None, group=None):
    """All-gather every rank's roll (G, E, W) -> (G, world*E, W) in global env order."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    G, E, W = roll.shape
    flat = torch.empty(world * G * E * W, dtype=roll.dtype, device=roll.device) if out is None else out
    dist.all_gather_into_tensor(flat, roll.contiguous().reshape(-1), group=group)
    return flat.reshape(world, G, E, W).permute(1, 0, 2, 3).reshape(G, world * E, W)
