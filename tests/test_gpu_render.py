"""The renderer on the GPU (include/avr.h avr_get_body_poses, avr_render_set_planes, avr_render_device)
against the float64 reference ray caster of tests/render_reference.py, through the C-ABI and the facade.

Tolerance (the project's 8x rule): on the pixels compared, |t_gpu - t_ref64| <= 8 max |t_ref32 - t_ref64|
over the same pixels, with one fp32 ulp of the largest t as the floor, where ref32 is the reference run
in float32 on the same inputs.  Observed on the MI355X: see DESIGN (the section on rendering)."""
import numpy as np
import pytest

from avr import _abi as ABI
from avr import _lib
from avr import render as RD

import render_reference as RR
import render_util as U

pytestmark = pytest.mark.gpu

PHASES = ('reset', 'stepped')
_SIM, _STATES, _SCENE = {}, {}, {}


def sim_of(task):
    """The task's 4-env handle with the hull planes installed (one per module run)."""
    if task not in _SIM:
        A, md = U.scene(task)
        _SIM[task] = _lib.Sim(md, U.N_ENVS, device=0)
        RD.install_planes(_SIM[task], A)
    return _SIM[task]


def states(task):
    """{'reset': the reset states, 'stepped': the states 20 random steps later}."""
    if task not in _STATES:
        sim = sim_of(task)
        S0 = U.reset_states(task)
        sim.set_state(S0)
        for t in range(20):
            sim.step(_lib.random_actions(1001, np.arange(U.N_ENVS), t))
        _STATES[task] = {'reset': S0, 'stepped': sim.get_state()}
    return _STATES[task]


def ref_scene(task):
    if task not in _SCENE:
        _SCENE[task] = RR.Scene(U.scene(task)[0])
    return _SCENE[task]


@pytest.fixture(scope='module', autouse=True)
def _close_handles():
    yield
    for s in _SIM.values():
        s.close()
    _SIM.clear()


def gender_of(md, row):
    return int(row[md.layout.S_TASK + md.layout.T_GENDER])


def ulp32(x):
    return float(np.spacing(np.float32(x)))


# ------------------------------------------------------------------ 1. body poses
@pytest.mark.parametrize('phase', PHASES)
@pytest.mark.parametrize('task', U.TASKS)
def test_body_poses_against_the_state_and_the_host_fk(task, phase):
    A, md = U.scene(task)
    L = md.layout
    sim = sim_of(task)
    S = states(task)[phase]
    sim.set_state(S)
    P = sim.body_poses()
    assert P.shape == (U.N_ENVS, sim.n_bodies(), 7) and sim.n_bodies() == len(A['body_kind'])
    bk, bi = np.asarray(A['body_kind']), np.asarray(A['body_index'])
    chain = set(int(x) for x in np.asarray(A['hc_slot']).ravel() if x >= 0) if 'hc_slot' in A else set()
    links = np.stack([sim.get_link_pose(l) for l in range(int(A['n_links']))], 1)     # [E, nl, 7]
    base = sim.get_link_pose(-1)
    st = np.asarray(A['st_pose'], np.float32).reshape(-1, 7)
    worst = worst_chain = 0.0
    for e in range(U.N_ENVS):
        hdyn = S[e, L.S_TASK + L.T_HDYN] != 0
        h64, h32 = U.host_body_poses(task, S[e]), U.host_body_poses(task, S[e], np.float32)
        for b in range(len(bk)):
            k, i = bk[b], bi[b]
            if k == ABI.BODY_ROBOT:
                assert np.array_equal(P[e, b], links[e, i]), (e, b)                # the same device function
                tol = max(8 * np.abs(h32[b].astype(np.float64) - h64[b]).max(), ulp32(np.abs(h64[b]).max()))
                err = np.abs(P[e, b] - h64[b]).max()
                worst = max(worst, err / tol)
                assert err <= tol, (e, b, err, tol)
            elif k == ABI.BODY_FREE:
                assert np.array_equal(P[e, b], S[e, L.S_FREE + ABI.FB_WORDS * i:L.S_FREE + ABI.FB_WORDS * i + 7]), (e, b)
            elif k == ABI.BODY_STATIC:
                assert np.array_equal(P[e, b], st[i]), (e, b)
            elif k == ABI.BODY_RSTATIC:
                assert np.array_equal(P[e, b], base[e]), (e, b)
            elif hdyn and i in chain:          # an articulated chain's slot: forward kinematics on the chain's joint words
                c64, c32 = U.chain_slot_poses(task, S[e])[i], U.chain_slot_poses(task, S[e], np.float32)[i]
                tol = max(8 * np.abs(c32.astype(np.float64) - c64).max(), ulp32(np.abs(c64).max()))
                err = np.abs(P[e, b] - c64).max()
                worst_chain = max(worst_chain, err / tol)
                assert err <= tol, (e, b, err, tol)
            else:
                assert np.array_equal(P[e, b], S[e, L.S_HUMAN + 7 * i:L.S_HUMAN + 7 * i + 7]), (e, b)
    print('%s %s: robot links within %.2f of the 8x bound, chain slots within %.2f' % (U.TASK_NAMES[task], phase, worst, worst_chain))
    if task == ABI.TASK_FEEDING and phase == 'stepped':    # the tremor env's head chain moved
        hb = RD.head_body(A, md)
        assert S[2, L.S_TASK + L.T_HDYN] != 0 and not np.array_equal(P[2, hb], sim_poses_at_reset(task)[2, hb])


def sim_poses_at_reset(task):
    sim = sim_of(task)
    sim.set_state(states(task)['reset'])
    return sim.body_poses()


# ------------------------------------------------------------------ 2. images against the reference
_CASES = {}


def image_case(task, name, phase):
    """Everything one image comparison needs: the GPU image of the case's env and the reference's
    (computed once per case and shared by the tests that read it)."""
    if (task, name, phase) not in _CASES:
        _CASES[task, name, phase] = _image_case(task, name, phase)
    return _CASES[task, name, phase]


def _image_case(task, name, phase):
    A, md = U.scene(task)
    sim = sim_of(task)
    S = states(task)[phase]
    sim.set_state(S)
    e = U.case_env(task, name)
    poses = sim.body_poses()[e]
    cam = U.case_camera(task, name, poses)
    out = RD.render_host(sim, A, cam, [e], ('depth', 'id', 'rgb'))
    sc, g = ref_scene(task), gender_of(md, S[e])
    t64, i64, n64, d64 = RR.trace(sc, g, poses, cam)
    t32, i32, n32, d32 = RR.trace(sc, g, poses, cam, np.float32)
    edge = RR.edge_pixels(sc, g, poses, cam)
    return dict(A=A, sc=sc, cam=cam, poses=poses, depth=out['depth'][0], id=out['id'][0], rgb=out['rgb'][0], t64=t64, i64=i64, n64=n64, d64=d64,
                t32=t32, i32=i32, n32=n32, d32=d32, edge=edge)


@pytest.mark.parametrize('phase', PHASES)
@pytest.mark.parametrize('name', U.CASES)
@pytest.mark.parametrize('task', U.TASKS)
def test_images_match_the_reference(task, name, phase):
    """Ids, depth (8x rule), conditioning, shading and misses on the non-edge pixels.  The conditions on
    how many pixels that must be are test_edge_share_and_coverage_conditions'."""
    C = image_case(task, name, phase)
    keep = ~C['edge']
    hit = keep & (C['i64'] >= 0)
    assert hit.any()
    # ids
    assert np.array_equal(C['id'][keep], C['i64'][keep]), 'ids differ on %d non-edge pixels' % (C['id'][keep] != C['i64'][keep]).sum()
    # depth: 8 x the float32 reference's own error over the same pixels, floor one ulp of t
    same32 = hit & (C['i32'] == C['i64'])
    with np.errstate(invalid='ignore'):          # (inf - inf on the pixels both miss; not selected)
        dt32, dtg = np.abs(C['t32'].astype(np.float64) - C['t64']), np.abs(C['depth'].astype(np.float64) - C['t64'])
    e32 = dt32[same32].max()
    bound = max(8 * e32, ulp32(C['t64'][hit].max()))
    err = dtg[hit].max()
    print('%s %s %s: %d non-edge hits, max |t_gpu - t_ref64| %.3g, bound %.3g (ratio %.2f), edge share %.3f'
          % (U.TASK_NAMES[task], name, phase, hit.sum(), err, bound, err / bound, C['edge'].mean()))
    assert bound < U.HULL_MARGIN, 'ill-conditioned inputs: the bound %.3g is not below the hull margin' % bound
    assert err <= bound
    # shading: the formula on the reference's normal; the float tolerance through the shade, plus one level for rounding
    s64 = RR.shade(C['n64'], C['d64'])
    s32 = RR.shade(C['n32'], C['d32']).astype(np.float64)
    want = RR.rgb_of(C['sc'], C['i64'], s64)
    # ... where a ray passes an edge between two faces of a box or hull closer than the depth bound, either
    # face's normal is within that tolerance: the shade may lie anywhere between theirs
    lo, hi = RR.facet_shade_range(C['sc'], C['poses'], C['cam'], C['i64'], C['d64'], bound)
    slack = np.fmax(np.fmax(s64 - lo, hi - s64), 0.0)
    slack = np.where(np.isnan(slack), 0.0, slack)
    tol = 255.0 * (max(8 * np.abs(s32 - s64)[same32].max(), ulp32(1.0)) + slack) + 1.0
    drgb = np.abs(C['rgb'].astype(np.float64) - want).max(-1)
    print('   shading: worst excess over the tolerance %.3g levels, %d pixels at a face edge within the depth bound'
          % ((drgb - tol)[hit].max(), (slack[hit] > 0).sum()))
    assert (drgb <= tol)[hit].all(), (drgb[hit].max(), tol[hit].min())
    # misses: exactly background, +inf and -1
    miss = keep & (C['i64'] < 0)
    assert (C['id'][miss] == -1).all() and np.isposinf(C['depth'][miss]).all() and (C['rgb'][miss] == np.array(RR.BACKGROUND, np.uint8)).all()
    assert C['depth'].dtype == np.float32 and C['id'].dtype == np.int32 and C['rgb'].dtype == np.uint8


def test_edge_share_and_coverage_conditions():
    """The conditions on the image test's inputs, at the poses the GPU gives, for every (task, camera,
    phase): at most 25 % edge pixels, at least 20 non-edge pixels on each of robot, human, static and
    tool / free bodies (tests/test_render_host.py checks the same at the reset states without a GPU and
    says how the views were chosen)."""
    bad = []
    for task in U.TASKS:
        for name in U.CASES:
            for phase in PHASES:
                C = image_case(task, name, phase)
                share, cov = float(C['edge'].mean()), U.coverage(C['A'], C['i64'], ~C['edge'])
                line = '%s %s %s: edge share %.3f, non-edge pixels %s' % (U.TASK_NAMES[task], name, phase, share, cov)
                print(line)
                if share > U.EDGE_CAP or min(cov.values()) < U.MIN_PIXELS:
                    bad.append(line)
    assert not bad, '\n'.join(bad)


# ------------------------------------------------------------------ 3. height variants
def test_height_variants_render_their_own_rows():
    from avr import model_compiler as MC
    from avr import reset as RS
    A, md = U.scene(ABI.TASK_FEEDING)
    L = md.layout
    heights = [0.50, 0.66]
    recs = [MC.human_variant_records('feeding_jaco', 'male', h) for h in heights]
    for R in recs:
        RD.assert_variant_hulls(A, R['arrays'])
    sim = _lib.Sim(md, 2, device=0)
    try:
        sim.human_variants_set(recs)
        ctx = dict(slots={'male': [2, 3], 'female': []}, pos={2 + v: R['human_pos'] for v, R in enumerate(recs)}, draw=None)
        S = np.concatenate([np.asarray(RS.batch_reset_states_fast(A, md, 1001, [0], genders=['male'], stream='philox',
                                                                  variants=dict(ctx, assign={0: 2 + v}))[0], np.float32) for v in range(2)])
        assert list(S[:, L.S_TASK + L.T_GENDER]) == [2.0, 3.0]
        sim.set_state(S)
        RD.install_planes(sim, A)
        P = sim.body_poses()
        cam = RD.default_camera(ABI.TASK_FEEDING, width=48, height=32)
        out = RD.render_host(sim, A, cam, None, ('depth', 'id'))
        assert not np.array_equal(out['id'][0], out['id'][1]) and not np.array_equal(out['depth'][0], out['depth'][1])
        base = ref_scene(ABI.TASK_FEEDING)
        for v in range(2):
            sc = base.with_rows(_rows(A, recs[v], 'shape_pose'), _rows(A, recs[v], 'shape_param'))
            t64, i64, _, _ = RR.trace(sc, 0, P[v], cam)
            t32, i32, _, _ = RR.trace(sc, 0, P[v], cam, np.float32)
            # the pixels whose four sub-pixel rays agree on the shape
            stable = ~(np.stack([RR.trace(sc, 0, P[v], cam, np.float64, sub)[1] for sub in RR.SUBS]) != i64).any(0)
            assert stable.mean() > 0.5 and np.array_equal(out['id'][v][stable], i64[stable])
            hit = stable & (i64 >= 0) & (i32 == i64)
            bound = max(8 * np.abs(t32.astype(np.float64) - t64)[hit].max(), ulp32(t64[hit].max()))
            assert np.abs(out['depth'][v].astype(np.float64) - t64)[hit].max() <= bound
            # the other variant's rows do not explain this image
            other = base.with_rows(_rows(A, recs[1 - v], 'shape_pose'), _rows(A, recs[1 - v], 'shape_param'))
            assert not np.array_equal(RR.trace(other, 0, P[v], cam)[1][stable], out['id'][v][stable])
    finally:
        sim.close()


def _rows(A, R, key):
    x = np.asarray(A[key], np.float64).copy()
    x[R['shapes']] = R[key]
    return x


# ------------------------------------------------------------------ 4. no side effect
def test_render_leaves_the_state_and_the_rollouts_untouched():
    import torch
    A, md = U.scene(ABI.TASK_FEEDING)
    S0 = np.tile(U.reset_states(ABI.TASK_FEEDING), (2, 1))
    n = len(S0)
    cam = RD.default_camera(ABI.TASK_FEEDING, width=48, height=32)
    dev = torch.device('cuda', 0)

    def run(with_render):
        sim = _lib.Sim(md, n, device=0)
        try:
            RD.install_planes(sim, A)
            sim.set_state(S0)
            obs = torch.zeros(4, n, md.layout.OBS_DIM, device=dev)
            rew, done, info = torch.zeros(4, n, device=dev), torch.zeros(4, n, dtype=torch.uint8, device=dev), torch.zeros(4, n, 2, device=dev)
            torch.cuda.synchronize()

            def roll(t0, k):
                sim.rollout_random_device(t0, k, obs[t0:].data_ptr(), rew[t0:].data_ptr(), done[t0:].data_ptr(), info[t0:].data_ptr(), stacked=True)
            roll(0, 2)
            sim.sync()
            caps = sim.graph_captures()
            if with_render:
                before = sim.get_state()
                img = RD.render_host(sim, A, cam, None, ('depth', 'id', 'rgb'))
                assert np.array_equal(sim.get_state().view(np.uint32), before.view(np.uint32))
                assert (img['id'] >= 0).any()
                assert sim.graph_captures() == caps
            roll(2, 2)
            sim.sync()
            return sim.get_state(), [x.cpu().numpy() for x in (obs, rew, done, info)], sim.graph_captures()
        finally:
            sim.close()
    a, b = run(False), run(True)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert a[2] == b[2]


# ------------------------------------------------------------------ 5. interface
def test_env_lists_single_outputs_and_repeatability():
    task = ABI.TASK_SCRATCH
    A, md = U.scene(task)
    sim = sim_of(task)
    sim.set_state(states(task)['stepped'])
    cam = RD.default_camera(task, width=50, height=29)          # (no multiple of the 8 x 8 tile)
    full = RD.render_host(sim, A, cam, None, ('depth', 'id', 'rgb'))
    assert full['depth'].shape == (4, 29, 50) and full['rgb'].shape == (4, 29, 50, 3)
    assert not np.array_equal(full['id'][0], full['id'][1])
    again = RD.render_host(sim, A, cam, None, ('depth', 'id', 'rgb'))
    for k in full:
        assert np.array_equal(full[k].view(np.uint8), again[k].view(np.uint8))
    ids = [3, 1, 1, 0, 3]
    perm = RD.render_host(sim, A, cam, ids, ('depth', 'id', 'rgb'))
    for k in full:
        assert np.array_equal(perm[k].view(np.uint8), full[k][ids].view(np.uint8))
    for k in full:
        assert np.array_equal(RD.render_host(sim, A, cam, None, (k,))[k].view(np.uint8), full[k].view(np.uint8))
    st = sim.render_tile_stats(cam)
    assert st.shape == (4, 4, 7, 2) and st[..., 0].max() <= len(A['shape_kind']) and st[..., 0].max() > 0
    info = sim.render_kernel_info()
    assert info['frames']['scratch_bytes'] == 0 and info['trace']['scratch_bytes'] == 0


def test_errors_leave_the_handle_usable():
    import dataclasses
    import torch
    task = ABI.TASK_BEDBATH
    A, md = U.scene(task)
    sim = sim_of(task)
    sim.set_state(states(task)['reset'])
    cam = RD.default_camera(task, width=48, height=32)
    good = RD.render_host(sim, A, cam, None, ('depth', 'id', 'rgb'))
    buf = torch.zeros(4 * 32 * 48, dtype=torch.float32, device='cuda:0')
    p = buf.data_ptr()
    R = dataclasses.replace
    cases = [(None, None, 'cam is NULL'), (R(cam, width=0), None, 'width and height'), (R(cam, height=4097), None, 'width and height'),
             (R(cam, fov_y_deg=0.0), None, 'fov_y_deg'), (R(cam, fov_y_deg=180.0), None, 'fov_y_deg'), (R(cam, near=0.0), None, 'near'),
             (R(cam, far=cam.near), None, 'near'), (R(cam, up=(0.0, 0.0, 0.0)), None, 'degenerate'), (R(cam, up=tuple(np.subtract(cam.target, cam.eye))), None, 'degenerate'),
             (R(cam, target=cam.eye), None, 'degenerate'), (cam, [0, 4], 'out of range'), (cam, [-1], 'out of range'),
             (R(cam, body=sim.n_bodies()), None, 'camera body'), (R(cam, body=-2), None, 'camera body')]
    for c, ids, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            sim.render_device(c, ids, p, None, None)
    with pytest.raises(RuntimeError, match='all NULL'):
        sim.render_device(cam, None, None, None, None)
    with pytest.raises(RuntimeError, match='out is NULL'):
        sim._chk(sim.lib.avr_get_body_poses(sim.h, None))
    again = RD.render_host(sim, A, cam, None, ('depth', 'id', 'rgb'))
    for k in good:
        assert np.array_equal(good[k].view(np.uint8), again[k].view(np.uint8))


def test_render_before_the_planes_is_an_error_and_plane_tables_are_checked():
    import torch
    A, md = U.scene(ABI.TASK_SCRATCH)
    sim = _lib.Sim(md, 1, device=0)
    try:
        sim.set_state(U.reset_states(ABI.TASK_SCRATCH)[:1])
        cam = RD.default_camera(ABI.TASK_SCRATCH, width=16, height=8)
        buf = torch.zeros(16 * 8, dtype=torch.int32, device='cuda:0')
        with pytest.raises(RuntimeError, match='avr_render_set_planes'):
            sim.render_device(cam, None, None, buf.data_ptr(), None)
        assert sim.body_poses().shape == (1, sim.n_bodies(), 7)      # (needs no planes)
        P, Rg = RD.hull_planes(A)
        hull = int(np.nonzero(Rg[:, 1] > 0)[0][0])
        for bad in (np.where(np.arange(len(Rg))[:, None] == hull, (0, 3), Rg), np.where(np.arange(len(Rg))[:, None] == hull, (len(P), 4), Rg),
                    np.where((Rg[:, 1] == 0)[:, None], (0, 1), Rg)):
            with pytest.raises(RuntimeError, match='plane range'):
                sim.render_set_planes(P, bad)
        with pytest.raises(RuntimeError, match='avr_render_set_planes'):
            sim.render_device(cam, None, None, buf.data_ptr(), None)
        sim.render_set_planes(P, Rg)
        sim.render_device(cam, None, None, buf.data_ptr(), None)
        sim.sync()
        assert (buf.cpu().numpy() >= 0).any()
    finally:
        sim.close()


def test_dressing_has_no_renderer():
    from avr import reset_dressing as RDR
    A = RDR.dressing_scene()
    md = ABI.ModelDesc(A)
    sim = _lib.Sim(md, 1, device=0)
    try:
        cam = _lib.Sim.camera_struct(RD.default_camera(ABI.TASK_FEEDING, width=8, height=8))
        import ctypes as C
        out = np.zeros(64, np.float32)
        assert sim.lib.avr_n_bodies(sim.h) == -1 and 'not built for DressingJaco' in sim.lib.avr_last_error(sim.h).decode()
        for rc in (sim.lib.avr_get_body_poses(sim.h, out.ctypes.data), sim.lib.avr_render_set_planes(sim.h, 0, None, out.ctypes.data),
                   sim.lib.avr_render_device(sim.h, C.byref(cam), 1, None, out.ctypes.data, None, None)):
            assert rc == -1 and sim.lib.avr_last_error(sim.h).decode() == 'render: not built for DressingJaco'
    finally:
        sim.close()


# ------------------------------------------------------------------ 6. facade
def test_facade_render_and_render_device():
    import torch
    from avr.env import AVREnv, AVRTorchVecEnv, AVRVecEnv
    env = AVRVecEnv('FeedingJaco-v0', 1, prefetch=False)
    try:
        env.reset()
        img = env.render()
        assert img.shape == (240, 320, 3) and img.dtype == np.uint8
        assert (img != np.array(RD.BACKGROUND, np.uint8)).any(2).mean() > 0.2
        both = env.render(width=64, height=48, outputs=('rgb', 'depth'), envs=[0, 0])
        assert both['rgb'].shape == (2, 48, 64, 3) and both['depth'].shape == (2, 48, 64) and np.array_equal(both['rgb'][0], both['rgb'][1])
        with pytest.raises(NotImplementedError):
            env.render(mode='human')
    finally:
        env.close()
    one = AVREnv('FeedingJaco-v0', impairment='none')
    try:
        one.reset()
        assert one.render(width=32, height=24).shape == (24, 32, 3)
    finally:
        one.close()
    tv = AVRTorchVecEnv('ScratchItchPR2-v0', 2, prefetch=False, auto_reset=False)
    try:
        tv.reset()
        a = torch.zeros(2, 7, device='cuda:0')
        tv.step(a)
        dev = tv.render_device(width=48, height=32, outputs=('rgb', 'depth', 'id'))      # queued behind the step, no host synchronisation
        tv.step(a)
        assert dev['rgb'].is_cuda and dev['rgb'].shape == (2, 32, 48, 3) and dev['id'].dtype == torch.int32
        S2 = tv.get_state()
        tv2 = AVRVecEnv('ScratchItchPR2-v0', 2, prefetch=False, auto_reset=False)
        try:
            tv2.reset()
            tv2.step(np.zeros((2, 7), np.float32))
            host = tv2.render(width=48, height=32, outputs=('rgb', 'depth', 'id'))
            for k in host:
                assert np.array_equal(dev[k].cpu().numpy().view(np.uint8), host[k].view(np.uint8)), k
        finally:
            tv2.close()
        assert S2.shape[0] == 2
    finally:
        tv.close()
