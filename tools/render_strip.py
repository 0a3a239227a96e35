#!/usr/bin/env python
"""A film strip of what a policy (or random actions) does: reset a task, step it, and write every
k-th frame of the chosen envs as PNGs plus one contact sheet (avr/render.py; include/avr.h
avr_render_device).  The debugging view of states that are otherwise dumps of numbers.

  python tools/render_strip.py --env FeedingJaco-v0 --envs 0,1 --steps 60 --every 10 --out strip/
  python tools/render_strip.py --env ScratchItchPR2-v0 --policy trained.pt --camera head

--camera: 'default' (the reference's GUI camera of the task), 'head' (the participant's view, riding
on the head's body) or 'tool' (a wrist camera riding on the tool's body, looking along the tool)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'assistive-vr-gym_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def camera(env, name):
    from avr import render as RD
    if name == 'default':
        return RD.default_camera(env.task)
    if name == 'head':        # 20 cm in front of the face, looking forward and down
        return RD.Camera.on_body(RD.head_body(env.A, env.md), (0.0, -0.20, 0.05), (0.0, -1.0, -0.45), (0.0, 0.0, 1.0), fov_y_deg=90.0)
    if name == 'tool':        # behind and above the tool's COM, looking at it
        return RD.Camera.on_body(int(env.md.desc.spoon_body), (0.0, -0.25, 0.25), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), fov_y_deg=70.0)
    raise SystemExit('unknown camera %r' % name)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--env', default='FeedingJaco-v0')
    ap.add_argument('--n-envs', type=int, default=4)
    ap.add_argument('--envs', default='0', help='comma-separated env indices to draw')
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--every', type=int, default=10, help='draw every k-th step (and the reset state)')
    ap.add_argument('--camera', default='default')
    ap.add_argument('--width', type=int, default=320)
    ap.add_argument('--height', type=int, default=240)
    ap.add_argument('--policy', default=None, help="a checkpoint avr.policy_eval.load_policy reads (default: the device's random actions)")
    ap.add_argument('--seed', type=int, default=1001)
    ap.add_argument('--out', default='strip')
    a = ap.parse_args()
    from avr import _lib, render as RD
    from avr.env import AVRVecEnv
    ids = [int(x) for x in a.envs.split(',')]
    os.makedirs(a.out, exist_ok=True)
    env = AVRVecEnv(a.env, a.n_envs, seed=a.seed, auto_reset=False, prefetch=False)
    try:
        obs = env.reset()
        act = None
        if a.policy:
            import torch
            from avr import policy_eval as PE
            ac, ob_rms = PE.load_policy(a.policy)

            def act(o):
                with torch.no_grad():
                    x = PE.normalize(torch.as_tensor(o, dtype=torch.float32), ob_rms)
                    return ac.act(x, None, None, deterministic=True)[1].clamp(-1.0, 1.0).numpy()
        cam = camera(env, a.camera)
        frames = []
        for t in range(a.steps + 1):
            if t % a.every == 0:
                rgb = env.render(envs=ids, camera=cam, width=a.width, height=a.height)
                for k, e in enumerate(ids):
                    RD.write_png(os.path.join(a.out, 'env%03d_step%04d.png' % (e, t)), rgb[k])
                frames.append(rgb)
            if t < a.steps:
                actions = act(obs) if act else _lib.random_actions(a.seed, env.env_offset + np.arange(env.n), t, env.L.ACT_DIM)
                obs = env.step(actions)[0]
        F = np.stack(frames, 1).reshape(-1, a.height, a.width, 3)      # one row per env, one column per drawn step
        RD.write_png(os.path.join(a.out, 'sheet.png'), RD.contact_sheet(F, cols=len(frames)))
        print('%d frames of envs %s -> %s (sheet.png: %d x %d)' % (len(frames), ids, a.out, len(ids), len(frames)))
    finally:
        env.close()


if __name__ == '__main__':
    main()
