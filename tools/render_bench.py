#!/usr/bin/env python
"""What a render costs and what bounds it, on one GPU, written to profiles/render.json:

  (a) rates    ms per call and frames per second of avr_render_device for `--envs` FeedingJaco envs at
               64 x 64 with depth + id, and for 1 env at 640 x 480 with all three outputs; and, for
               scale, the ms of one env-step of the same handle (a 16-step random rollout / 16).  The
               three are timed interleaved over --repeats repeats with HIP events on the handle's stream
               after an untimed pass; medians, every sample and the spread (max - min over the median).
  (b) culling  per 8 x 8 tile the shapes its culled list holds and the hull planes one of its pixels tests
               (avr_render_tile_stats), mean and maximum, against the uncut counts (every shape of the
               env's gender, every plane of their hulls).
  (c) step     the rollout rate with a render between rollouts against the rate without, interleaved in
               the same process: the render queues behind the step on the handle's stream and takes
               nothing from it but its own time.

One JSON line is printed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'assistive-vr-gym_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def summary(x):
    med = statistics.median(x)
    return dict(median=med, min=min(x), max=max(x), spread=(max(x) - min(x)) / med, samples=x)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render.json'))
    a = ap.parse_args()
    import numpy as np
    import torch
    from avr import _abi as ABI, render as RD
    from avr.env import AVRTorchVecEnv
    E = a.envs
    env = AVRTorchVecEnv('FeedingJaco-v0', E, auto_reset=False)
    try:
        env.reset()
        sim, dev, A = env.sim, env.dev, env.A
        RD.install_planes(sim, A)
        small = RD.default_camera(ABI.TASK_FEEDING, width=64, height=64)
        big = RD.default_camera(ABI.TASK_FEEDING, width=640, height=480)
        d_s = torch.empty(E, 64, 64, device=dev)
        i_s = torch.empty(E, 64, 64, dtype=torch.int32, device=dev)
        d_b = torch.empty(1, 480, 640, device=dev)
        i_b = torch.empty(1, 480, 640, dtype=torch.int32, device=dev)
        c_b = torch.empty(1, 480, 640, 3, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        S = env.get_state()
        ext = env.ext

        def timed(fn):
            with torch.cuda.stream(ext):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(ext)
                fn()
                t1.record(ext)
            t1.synchronize()
            return t0.elapsed_time(t1)

        runs = dict(small=lambda: sim.render_device(small, None, d_s.data_ptr(), i_s.data_ptr(), None),
                    big=lambda: sim.render_device(big, [0], d_b.data_ptr(), i_b.data_ptr(), c_b.data_ptr()),
                    steps16=lambda: sim.rollout_random_device(0, 16),
                    steps16_render=lambda: (sim.rollout_random_device(0, 16), sim.render_device(small, None, d_s.data_ptr(), i_s.data_ptr(), None)))
        ms = {k: [] for k in runs}
        for rep in range(a.repeats + 1):
            for k, fn in runs.items():
                env.set_state(S)
                t = timed(fn)
                if rep:                     # (the first pass captures graphs and grows the scratch)
                    ms[k].append(t)
        R = {k: summary(v) for k, v in ms.items()}
        step_ms = R['steps16']['median'] / 16
        rates = dict(small=dict(envs=E, size=[64, 64], outputs=['depth', 'id'], ms_per_call=R['small'], frames_per_s=E / R['small']['median'] * 1e3),
                     big=dict(envs=1, size=[640, 480], outputs=['depth', 'id', 'rgb'], ms_per_call=R['big'], frames_per_s=1e3 / R['big']['median']),
                     env_step_ms=step_ms, small_render_in_env_steps=R['small']['median'] / step_ms)
        env.set_state(S)
        n_st = min(E, 64)
        st = sim.render_tile_stats(small, list(range(n_st))).reshape(n_st, -1, 2).astype(np.float64)
        P, Rg = RD.hull_planes(A)
        g = S[:n_st, env.L.S_TASK + env.L.T_GENDER].astype(int) % 2
        sg = np.asarray(A['shape_gender'])
        on = [(sg < 0) | (sg == x) for x in g]
        cull = dict(envs=n_st, list_mean=st[..., 0].mean(), list_max=st[..., 0].max(), shapes_uncut=float(np.mean([m.sum() for m in on])),
                    planes_mean=st[..., 1].mean(), planes_max=st[..., 1].max(), planes_uncut=float(np.mean([Rg[m, 1].sum() for m in on])))
        plain = E * 16 / statistics.median(ms['steps16']) * 1e3
        with_r = E * 16 / statistics.median(ms['steps16_render']) * 1e3
        step = dict(env_steps_per_s_plain=plain, env_steps_per_s_with_a_render_every_16=with_r, plain_ms=R['steps16'], with_render_ms=R['steps16_render'],
                    render_share_ms=R['steps16_render']['median'] - R['steps16']['median'])
        out = dict(tool='render_bench', env='FeedingJaco-v0', kernels=sim.render_kernel_info(), rates=rates, culling=cull, step=step)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
    finally:
        env.close()


if __name__ == '__main__':
    main()
