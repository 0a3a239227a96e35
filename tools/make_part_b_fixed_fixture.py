"""Writes tests/golden/part_b_fixed_feeding.npz, the FeedingJaco states of tests/test_part_b_fixed.py,
on the CPU with the fp64 oracle: 64 reset states (seed 1001, impairment 'random'), 100 settle frames
and 29 gym steps of Philox random actions, when the food has been thrown about and some envs hold
well over 43 contacts.  37 of them are laid out over part B's blocks (block x holds envs x, x + 8,
x + 16, x + 24; envs 32-36 sit alone in theirs):

  envs 1, 2, 4, 5   the four states with the most contacts, so blocks 1, 2, 4 and 5 each stage more
                    records for one group than 32 loads per lane hold
  every third env   its raw reset state with the bowl and the food far from the scene: no contact
  env 17            (block 1) all but three food pieces far from the scene: a few contacts
  the others        contact-rich states in source order

    python tools/make_part_b_fixed_fixture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'assistive-vr-gym_amd'))
sys.path.insert(0, ROOT)

N_SRC, N, STEPS = 64, 37, 29
BIG_SLOTS, FEW = (1, 2, 4, 5), 17


def far(S, d, e, frees):
    from avr import _abi as ABI
    for f in frees:
        o = ABI.S_FREE + ABI.FB_WORDS * f
        S[e, o:o + 3] = (50.0 + 2.0 * f, 50.0, 1.0)
        S[e, o + 7:o + 13] = 0.0


def main():
    from avr import _abi as ABI, _lib, reset as RS
    from oracle.oracle import Oracle
    A = ABI.load_scene()
    md = ABI.ModelDesc(A)
    d = md.desc
    R, _ = RS.batch_reset_states_fast(A, md, 1001, list(range(N_SRC)), impairment='random')
    o = Oracle(md, N_SRC)
    o.set_state(R)
    o.settle(100)
    for k in range(STEPS):
        o.step(_lib.random_actions(1001, np.arange(N_SRC), k))
    G = o.get_state()
    o.close()
    ncp = G[:, ABI.S_TASK + ABI.T_NCP].astype(int)
    order = np.argsort(-ncp, kind='stable')
    big = order[:len(BIG_SLOTS)].tolist()
    rest = [e for e in range(N_SRC) if e not in big]
    S = np.zeros((N, G.shape[1]))
    src = []
    for e in range(N):
        s = big[BIG_SLOTS.index(e)] if e in BIG_SLOTS else rest.pop(0)
        S[e] = G[s]
        src.append(s)
    food = list(range(d.food_free0, d.food_free0 + d.n_food))
    cp = slice(ABI.S_CP, ABI.S_CP + ABI.MAX_CONTACTS * ABI.CP_WORDS)
    for e in range(0, N, 3):
        S[e] = R[e]
        far(S, d, e, [d.bowl_free] + food)
    far(S, d, FEW, food[3:])
    S[FEW, cp] = 0.0            # (its cached contacts went with the food)
    S[FEW, ABI.S_TASK + ABI.T_NCP] = 0.0
    out = os.path.join(ROOT, 'tests', 'golden', 'part_b_fixed_feeding.npz')
    np.savez_compressed(out, S=S.astype(np.float32), src=np.array(src, np.int32))
    print(out, os.path.getsize(out), 'bytes; source contacts', ncp[src].tolist())


if __name__ == '__main__':
    main()
