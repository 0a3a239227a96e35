"""Diagnostic: the bench's FeedingJaco workload (4096 envs, the bench's reset pool, 100 settle frames,
device-random steps) on three handles in lockstep -- AVR_PAIRS_FLAT=0, 1 and 1 again -- comparing
every step's outputs bit for bit, and the final states.  On a difference it replays from the last
checkpoint with state compares, saves the first differing env's pre-step state, and replays that
env alone, step and sub-steps, on both paths.

    python tools/front_end_lockstep.py [steps (500)] [out dir (bench_out/lockstep)]
"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'assistive-vr-gym_amd')); sys.path.insert(0, ROOT)
import torch
from avr import _abi as ABI, _lib
import bench
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'bench_out', 'lockstep'); os.makedirs(OUT, exist_ok=True)
T = int(sys.argv[1]) if len(sys.argv) > 1 else 500
E = 4096
A = ABI.load_scene(0); md = ABI.ModelDesc(A); L = md.layout
S_pool, meta = bench.reset_pool(0, A, md, list(range(1024)), 'random')
S = np.tile(S_pool, (4, 1))[:E].astype(np.float32)
def mk(flat, n=E):
    os.environ['AVR_PAIRS_FLAT'] = str(flat)
    s = _lib.Sim(md, n, seed=1001)
    os.environ.pop('AVR_PAIRS_FLAT')
    assert s.pairs_flat() == flat
    return s
sims = [mk(0), mk(1), mk(1)]
dev = torch.device('cuda', 0)
bufs = []
for s in sims:
    s.set_state(S); s.settle(100)
    bufs.append((torch.zeros(E, L.OBS_DIM, device=dev), torch.zeros(E, device=dev), torch.zeros(E, dtype=torch.uint8, device=dev), torch.zeros(E, L.INFO_DIM, device=dev)))
G0 = [s.get_state() for s in sims]
print('after settle: 0v1 equal', np.array_equal(G0[0].view(np.uint32), G0[1].view(np.uint32)), '1v2 equal', np.array_equal(G0[1].view(np.uint32), G0[2].view(np.uint32)), flush=True)
CK = 8
ck = (0, G0[0])
first = None
for t in range(T):
    if t % CK == 0 and t:
        ck = (t, sims[0].get_state())
    for s, b in zip(sims, bufs):
        s.step_random_device(t, *[x.data_ptr() for x in b])
    for s in sims: s.sync()
    torch.cuda.synchronize()
    e01 = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(bufs[0], bufs[1]))
    e12 = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(bufs[1], bufs[2]))
    if not (e01 and e12):
        first = t
        print('step %d: flat0 v flat1 equal %s, flat1 v flat1 equal %s' % (t, e01, e12), flush=True)
        break
if first is None:
    print('no difference in %d steps' % T)
    Gs = [s.get_state() for s in sims]
    print('final states 0v1', np.array_equal(Gs[0].view(np.uint32), Gs[1].view(np.uint32)), '1v2', np.array_equal(Gs[1].view(np.uint32), Gs[2].view(np.uint32)))
    sys.exit(0)
# replay from the checkpoint with state compares
t0, P = ck
for s in sims: s.set_state(P)
env = None
for t in range(t0, first + 1):
    pre = sims[0].get_state()
    for s, b in zip(sims, bufs):
        s.step_random_device(t, *[x.data_ptr() for x in b]); s.sync()
    Gs = [s.get_state().view(np.uint32) for s in sims]
    d01 = np.nonzero((Gs[0] != Gs[1]).any(1))[0]; d12 = np.nonzero((Gs[1] != Gs[2]).any(1))[0]
    print('replay step %d: envs differing 0v1 %s, 1v2 %s' % (t, d01[:10], d12[:10]), flush=True)
    if len(d01) or len(d12):
        env = int((d01 if len(d01) else d12)[0]); break
if env is None:
    print('replay from the checkpoint did not reproduce the difference'); sys.exit(0)
w = np.nonzero(Gs[0][env] != Gs[1][env])[0]
print('env %d step %d: %d state words differ, first %s; flags %s / %s' % (env, t, len(w), w[:12], sims[0].get_flags()[env], sims[1].get_flags()[env]))
np.savez(os.path.join(OUT, 'diff.npz'), pre=pre[env], t=t, env=env, post0=Gs[0][env], post1=Gs[1][env])
for s in sims: s.close()
# small replay: the env's pre-step state in 8 slots, host action of (env, t); then plain sub-steps
n = 8
Pn = np.tile(pre[env], (n, 1))
act = np.tile(_lib.random_actions(1001, np.array([env]), t), (n, 1)).astype(np.float32)
res = []
for flat in (0, 1):
    s = mk(flat, n); s.set_state(Pn); s.step(act); res.append((s.get_state().view(np.uint32), s.get_flags())); s.close()
print('small replay step: equal %s (flags %s %s); matches big flat0 %s' % (np.array_equal(res[0][0], res[1][0]), res[0][1][:2], res[1][1][:2], np.array_equal(res[0][0][0], Gs[0][env])))
a, b = mk(0, n), mk(1, n)
a.set_state(Pn); b.set_state(Pn)
for k in range(12):
    pa = a.get_state()
    a.substep(0.005); b.substep(0.005)
    ga, gb = a.get_state().view(np.uint32), b.get_state().view(np.uint32)
    eq = np.array_equal(ga, gb)
    print('sub-step %d equal %s flags %s %s' % (k, eq, a.get_flags()[0], b.get_flags()[0]), flush=True)
    if not eq:
        np.save(os.path.join(OUT, 'substep_pre.npy'), pa[0])
        print('words differing', np.nonzero(ga[0] != gb[0])[0][:20])
        break
