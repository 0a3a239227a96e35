"""Diagnostic: where a cooperative pair's time goes (AVR_PROF build, libavr_prof.so) -- the cycles inside
its support queries against its total, the number of queries, and the env's slowest pair, in the
bench workload's launch shape (FeedingJaco, N envs in the default env groups, after the 100-frame
settle).  AVR_COOP_WSUP=0|1 in the environment selects the serial or the wave-wide supports.

    python tools/coop_support_prof.py OUT.json [N=4096] [STEPS=3]
"""
import ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'assistive-vr-gym_amd')); sys.path.insert(0, ROOT)
from avr import _abi as ABI, reset as RS, _lib
so = os.path.join(ROOT, 'assistive-vr-gym_amd', 'avr', 'libavr_prof.so')
_lib.LIB_PATH = so
lib = _lib.load(so)
lib.avr_set_profile_buffer.argtypes = [C.c_void_p, C.c_void_p]
import torch
N = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
A = ABI.load_scene(0); md = ABI.ModelDesc(A)
S, _ = RS.batch_reset_states_fast(A, md, 1001, list(range(min(N, 256))), impairment='random')
S = np.tile(S, ((N + len(S) - 1) // len(S), 1))[:N]
sim = _lib.Sim(md, N)
SLOTS = 64
prof = torch.zeros(N * SLOTS, dtype=torch.int64, device='cuda')
lib.avr_set_profile_buffer(sim.h, prof.data_ptr())
sim.set_state(S.astype(np.float32)); sim.settle(100)
NSUB = 10
rec = dict(what='tools/coop_support_prof.py, AVR_PROF build, FeedingJaco, %d envs in %d groups, coop_wsup %d; cycles; per gym step' % (N, sim.env_groups(), sim.coop_wsup()), steps=[])
for t in range(STEPS):
    prof.zero_(); torch.cuda.synchronize()
    sim.step(_lib.random_actions(1001, np.arange(N), t))
    p = prof.cpu().numpy().reshape(N, SLOTS)
    pairs, cyc, sup, nq, its = p[:, 11].sum(), p[:, 29].sum(), p[:, 23].sum(), p[:, 31].sum(), p[:, 28].sum()
    slow = p[:, 47].astype(np.uint64)                   # per env: cycles << 36 | support cycles << 12 | queries of its slowest pair
    sc, ss, sq = (slow >> np.uint64(36)).astype(np.int64), ((slow >> np.uint64(12)) & np.uint64(0xffffff)).astype(np.int64), (slow & np.uint64(0xfff)).astype(np.int64)
    has = sc > 0
    top = np.argsort(-sc)[:10]
    rec['steps'].append(dict(
        coop_pairs=int(pairs), envs_with_a_pair=int(has.sum()), pairs_per_env_and_substep=float(pairs) / N / NSUB,
        by_kind=dict(sphere_hull=int(p[:, 19].sum()), hull_hull=int(p[:, 20].sum()), other=int(p[:, 21].sum()), big_hull_without_table=int(p[:, 22].sum())),
        cycles_per_pair=float(cyc) / max(pairs, 1), support_cycles_per_pair=float(sup) / max(pairs, 1), support_share=float(sup) / max(cyc, 1),
        queries_per_pair=float(nq) / max(pairs, 1), cycles_per_query=float(sup) / max(nq, 1), gjk_iterations_per_pair=float(its) / max(pairs, 1),
        max_table_cell_candidates=int(p[:, 5].max()),
        slowest_pair_per_env=dict(mean_cycles=float(sc[has].mean()) if has.any() else 0.0, p99_cycles=float(np.percentile(sc[has], 99)) if has.any() else 0.0,
                                  max_cycles=int(sc.max()), mean_support_share=float((ss[has] / np.maximum(sc[has], 1)).mean()) if has.any() else 0.0,
                                  ten_slowest=[dict(cycles=int(sc[e]), support_cycles=int(ss[e]), queries=int(sq[e])) for e in top]),
        kernel_a_cycles_of_envs=dict(with_a_pair=float((p[has, 3] + p[has, 8]).mean()) if has.any() else 0.0, without=float((p[~has, 3] + p[~has, 8]).mean()))))
    print(json.dumps(rec['steps'][-1])[:600])
sim.close()
json.dump(rec, open(sys.argv[1], 'w'), indent=1)
