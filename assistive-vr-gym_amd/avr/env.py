"""Gym-style facade over libavr: the reference's reset/step contract, batched.

Reference contract being mirrored:
  * ids registered in assistive_gym/__init__.py (FeedingJaco-v0 -> FeedingJacoEnv,
    ScratchItchPR2-v0 -> ScratchItchPR2Env; TimeLimit 200);
  * reset() -> obs: FeedingJaco (25,), feeding.py:144-331 (scene randomisation, IK, 100 food-drop
    frames); ScratchItchPR2 (30,), scratch_itch.py:130-273 (base-pose search + IK, no settle);
  * step(a) -> (obs, reward, done, info) with info keys total_force_on_human, task_success,
    action_robot_len, action_human_len, obs_robot_len, obs_human_len (feeding.py:76,
    scratch_itch.py:78); done at iteration >= 200 (TimeLimit).
  * observation/action spaces: Box(-1e9, 1e9, (obs,)) and Box(-1, 1, (7,)), float32 (env.py:34-35).

AVRVecEnv steps all envs of one GPU in one launch sequence (host arrays in/out); AVRTorchVecEnv
is the same with device tensors (no host copies per step); AVREnv is the single-env view
(n_envs=1) that reads like `gym.make('FeedingJaco-v0')`.  Physics runs only on the GPU (libavr);
there is no CPU fallback here.

Episode rollover (auto_reset): FeedingJaco resets run the IK on the device (avr_reset_ik) from
the host's reset draws (reset.reset_inputs), which a background thread prepares for the next
episode while the current one steps; ScratchItch resets run the host base-pose search + IK
(reset_scratch.batch_reset_states), then avr_reset.
"""
import sys
import threading
import time

import numpy as np

from . import _abi as ABI
from . import _lib
from . import render as RD
from . import reset as RS

MAX_EPISODE_STEPS = 200          # assistive_gym/__init__.py TimeLimit
# settle frames after the reset state is in place: feeding.py:318-320; scratch_itch.py has none;
# bed_bathing.py's 100-frame arm settle (:288-289) comes before the robot is placed (reset_bedbath)
SETTLE_FRAMES = {ABI.TASK_FEEDING: 100, ABI.TASK_SCRATCH: 0, ABI.TASK_BEDBATH: 0, ABI.TASK_DRESSING: 0}


class Box:
    """Minimal stand-in for gym.spaces.Box (gym is not a dependency of this package)."""

    def __init__(self, low, high, shape, dtype=np.float32):
        self.low = np.full(shape, low, dtype)
        self.high = np.full(shape, high, dtype)
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)

    def sample(self, rng=None):
        rng = rng or np.random.default_rng()
        return rng.uniform(self.low, self.high).astype(self.dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))

    def __repr__(self):
        return 'Box(%s, %s, %s, %s)' % (self.low.min(), self.high.max(), self.shape, self.dtype)


# id -> (task, robot, implemented): every id the reference registers (assistive_gym/__init__.py);
# this build implements FeedingJaco-v0, ScratchItchPR2-v0 and BedBathingPR2-v0, the
# rest raise NotImplementedError.
REGISTRY = {
    'HumanTesting-v0':           ('human_testing', '-', False),
    'ScratchItchPR2-v0':         ('scratch_itch', 'pr2', True),
    'ScratchItchJaco-v0':        ('scratch_itch', 'jaco', False),
    'ScratchItchPR2Human-v0':    ('scratch_itch', 'pr2', False),
    'ScratchItchJacoHuman-v0':   ('scratch_itch', 'jaco', False),
    'ScratchItchPR2New-v0':      ('scratch_itch', 'pr2', False),
    'ScratchItchJacoNew-v0':     ('scratch_itch', 'jaco', False),
    'ScratchItchVRPR2-v0':       ('scratch_itch', 'pr2', False),
    'ScratchItchVRJaco-v0':      ('scratch_itch', 'jaco', False),
    'ScratchItchVRPR2Human-v0':  ('scratch_itch', 'pr2', False),
    'ScratchItchVRJacoHuman-v0': ('scratch_itch', 'jaco', False),
    'ScratchItchVRPR2New-v0':    ('scratch_itch', 'pr2', False),
    'ScratchItchVRJacoNew-v0':   ('scratch_itch', 'jaco', False),
    'BedBathingPR2-v0':          ('bed_bathing', 'pr2', True),
    'BedBathingJaco-v0':         ('bed_bathing', 'jaco', False),
    'BedBathingPR2Human-v0':     ('bed_bathing', 'pr2', False),
    'BedBathingJacoHuman-v0':    ('bed_bathing', 'jaco', False),
    'BedBathingPR2New-v0':       ('bed_bathing', 'pr2', False),
    'BedBathingJacoNew-v0':      ('bed_bathing', 'jaco', False),
    'BedBathingVRPR2-v0':        ('bed_bathing', 'pr2', False),
    'BedBathingVRJaco-v0':       ('bed_bathing', 'jaco', False),
    'BedBathingVRPR2Human-v0':   ('bed_bathing', 'pr2', False),
    'BedBathingVRJacoHuman-v0':  ('bed_bathing', 'jaco', False),
    'BedBathingVRPR2New-v0':     ('bed_bathing', 'pr2', False),
    'BedBathingVRJacoNew-v0':    ('bed_bathing', 'jaco', False),
    'DrinkingPR2-v0':            ('drinking', 'pr2', False),
    'DrinkingJaco-v0':           ('drinking', 'jaco', False),
    'DrinkingPR2Human-v0':       ('drinking', 'pr2', False),
    'DrinkingJacoHuman-v0':      ('drinking', 'jaco', False),
    'DrinkingPR2New-v0':         ('drinking', 'pr2', False),
    'DrinkingJacoNew-v0':        ('drinking', 'jaco', False),
    'DrinkingVRPR2-v0':          ('drinking', 'pr2', False),
    'DrinkingVRJaco-v0':         ('drinking', 'jaco', False),
    'DrinkingVRPR2Human-v0':     ('drinking', 'pr2', False),
    'DrinkingVRJacoHuman-v0':    ('drinking', 'jaco', False),
    'DrinkingVRPR2New-v0':       ('drinking', 'pr2', False),
    'DrinkingVRJacoNew-v0':      ('drinking', 'jaco', False),
    'FeedingPR2-v0':             ('feeding', 'pr2', False),
    'FeedingJaco-v0':            ('feeding', 'jaco', True),
    'FeedingPR2Human-v0':        ('feeding', 'pr2', False),
    'FeedingJacoHuman-v0':       ('feeding', 'jaco', False),
    'FeedingPR2New-v0':          ('feeding', 'pr2', False),
    'FeedingJacoNew-v0':         ('feeding', 'jaco', False),
    'FeedingVRPR2-v0':           ('feeding', 'pr2', False),
    'FeedingVRJaco-v0':          ('feeding', 'jaco', False),
    'FeedingVRPR2Human-v0':      ('feeding', 'pr2', False),
    'FeedingVRJacoHuman-v0':     ('feeding', 'jaco', False),
    'FeedingVRPR2New-v0':        ('feeding', 'pr2', False),
    'FeedingVRJacoNew-v0':       ('feeding', 'jaco', False),
    # BASELINE.json configs[4]; not registered by the reference (it has no dressing task, SURVEY
    # 0.5): a build-defined task on the reference's dressing hooks (include/avr_dressing.h)
    'DressingJaco-v0':           ('dressing', 'jaco', True),
}

# The registry's flag counts the ids with a compiled scene and task glue of their own.  Ids that run
# on another id's build with a reset of their own are built too: id -> the id whose build they use.
# FeedingJacoNew-v0 is FeedingJaco-v0's scene and kernels with the `new` reset (feeding.py:168-246);
# the other New ids stay NotImplementedError.
BUILT_ON = {'FeedingJacoNew-v0': 'FeedingJaco-v0'}


def is_built(env_id):
    return env_id in BUILT_ON or REGISTRY[env_id][2]


_SCENES = {}
_TASK_OF = {'feeding': ABI.TASK_FEEDING, 'scratch_itch': ABI.TASK_SCRATCH, 'bed_bathing': ABI.TASK_BEDBATH, 'dressing': ABI.TASK_DRESSING}


def _scene(task, heights=None):
    """(arrays, ModelDesc) of a task's scene with the human at per-gender hipbone_to_mouth_height
    `heights` (None: the defaults, the committed npz; otherwise rebuilt by the model compiler
    from its asset cache, human_creation.py:60-63,75)."""
    from . import model_compiler as MC
    H = MC.human_heights(heights)
    key = (task,) + tuple(H[g] for g in ('male', 'female'))
    if key not in _SCENES:
        if task == 'dressing':
            if not MC.default_heights(H):
                raise NotImplementedError('DressingJaco-v0: only the default human proportions are built')
            from . import reset_dressing as RD
            A = RD.dressing_scene()
        elif MC.default_heights(H):
            A = ABI.load_scene(_TASK_OF[task])
        else:
            A = MC.scene_arrays(ABI.SCENES[_TASK_OF[task]], H)
        _SCENES[key] = (A, ABI.ModelDesc(A))
    return _SCENES[key]


def variant_table(human_heights):
    """The height variants a human_heights argument asks for: None when every entry is a scalar (one
    rebuilt scene, no variants), else [(gender, height), ...] -- the male list, then the female
    list; variant v is proportions slot 2 + v (include/avr.h avr_human_variants_set).  Raises
    ValueError for an unknown gender, a height outside model_compiler.human_heights' [0.3, 1.0] or
    more than 64 variants."""
    from . import model_compiler as MC
    out, any_list = [], False
    for g in (human_heights or {}):
        if g not in MC.DEFAULT_HEIGHT:
            raise ValueError('heights: gender must be male or female, got %r' % (g,))
    for g in MC.GENDERS:
        v = (human_heights or {}).get(g)
        if isinstance(v, (list, tuple, np.ndarray)):
            any_list = True
            if not len(v):
                raise ValueError('human_heights[%r]: an empty list of heights' % g)
            out += [(g, MC.human_heights({g: float(h)})[g]) for h in v]
    if not any_list:
        return None
    if len(out) > MC.MAX_HUMAN_VARIANTS:
        raise ValueError('%d height variants: a handle holds at most %d' % (len(out), MC.MAX_HUMAN_VARIANTS))
    return out


def new_height_grid():
    """FeedingJacoNew-v0's heights: 21 values per gender over [default - 0.1, default + 0.1] in 1 cm
    steps (the reference draws a continuous height there, feeding.py:170-172)."""
    from . import model_compiler as MC
    return {g: [round(MC.DEFAULT_HEIGHT[g] + 0.01 * k, 2) for k in range(-10, 11)] for g in MC.GENDERS}


class _Prefetch:
    """Reset draws of the next episode of a set of envs, prepared on a background thread while
    the stepping thread keeps the GPU fed.  The stepping thread takes and drops the GIL around
    every ctypes / torch call; at the default 5 ms switch interval a GIL-bound worker would delay
    each re-acquisition by up to 5 ms and starve the launches, so the interval is lowered to
    0.1 ms while the worker runs."""

    def __init__(self, fn):
        self.fn = fn
        self.key = None
        self.result = None
        self.thread = None

    def start(self, key, *args):
        self.wait()
        self.key, self.result = key, None

        def run():
            old = sys.getswitchinterval()
            sys.setswitchinterval(1e-4)
            try:
                self.result = self.fn(*args)
            finally:
                sys.setswitchinterval(old)
        self.thread = threading.Thread(target=run, daemon=True)
        self.thread.start()

    def wait(self):
        if self.thread is not None:
            self.thread.join()
            self.thread = None

    def take(self, key):
        self.wait()
        if self.key == key and self.result is not None:
            r, self.key, self.result = self.result, None, None
            return r
        return None


class AVRVecEnv:
    """n_envs environments of one task on one GPU; host arrays in and out.

    env_offset: global id of env 0 (multi-GPU sharding: rank * n_envs); reset randomness and the
    synthetic action stream are keyed by the global env id, so results do not depend on how
    envs are split over GPUs.

    impairment: 'random' (the tasks' own setting, feeding.py:175 / scratch_itch.py:178: none /
    limits / weakness / tremor, one draw per episode), a fixed one of those four, or 'no_tremor'.
    reset_ik: 'device' (default: FeedingJaco's and DressingJaco's IK through avr_reset_ik, the PR2
    tasks' base-pose search through avr_base_search) or 'host' (the fp64 host restatements, then
    avr_reset).
    reset_stream: FeedingJaco's reset draws, 'philox' (counter-based, vectorised; default) or
    'numpy' (the per-env Generator stream of the bench's reset pools and the golden fixtures).
    human_heights: the human's proportions, {gender: hipbone_to_mouth_height} (create_human's
    hmhs = height / 0.6 male, / 0.54 female, human_creation.py:60-63: capsule lengths and joint
    offsets scale by it, BedBathing's wipe targets too, bed_bathing.py:359-370); a gender not
    named keeps its default.  A scalar is one rebuilt scene for the handle: the reference builds
    its human at the height the env holds (a replay's setup.pkl, feeding.py:153-156; setup(),
    feeding.py:20-28).  A list per gender, {'male': [...], 'female': [...]}, loads the heights as
    variants of the one handle (include/avr.h avr_human_variants_set, at most 64 in all; FeedingJaco
    with the 'philox' reset stream): every env then has its own person per episode.
    height_draw: 'uniform' (default) draws the env's variant among its gender's list per env and
    episode from the reset's counter-based stream (keyed by global env id and episode, so it does
    not depend on env_offset sharding); None uses the list's first height.  proportions() returns
    every env's gender and height.
    """

    def __init__(self, env_id='FeedingJaco-v0', n_envs=1, device=0, seed=1001, env_offset=0, auto_reset=True,
                 impairment='random', reset_ik='device', prefetch=True, scratch_attempts=100, scratch_iters=200,
                 reset_stream='philox', human_heights=None, height_draw='uniform'):
        if env_id not in REGISTRY:
            raise KeyError('unknown env id %r' % env_id)
        task, robot, _ = REGISTRY[env_id]
        if not is_built(env_id):
            raise NotImplementedError('%s: only FeedingJaco-v0, FeedingJacoNew-v0, ScratchItchPR2-v0, BedBathingPR2-v0 and DressingJaco-v0 are built (SURVEY 8)' % env_id)
        if height_draw not in ('uniform', None):
            raise ValueError("height_draw must be 'uniform' or None, not %r" % (height_draw,))
        # FeedingJacoNew-v0 (feeding.py:168-246, the `new` branches): a new height per episode from a
        # 1 cm grid (human_heights overrides it), impairment 'none', waist and head draws, the
        # human-robot clearance redraw loop
        self.new = env_id == 'FeedingJacoNew-v0'
        if self.new:
            if reset_ik != 'device' or reset_stream != 'philox':
                raise NotImplementedError("FeedingJacoNew-v0 resets through the device IK and the 'philox' stream")
            human_heights = new_height_grid() if human_heights is None else human_heights
            impairment = 'none'
        self.env_id = env_id
        self.n = int(n_envs)
        self.seed = int(seed)
        self.env_offset = int(env_offset)
        self.auto_reset = auto_reset
        self.impairment = impairment
        from . import model_compiler as MC
        self.variants = variant_table(human_heights)          # None, or [(gender, height)]: slot 2 + v
        self.height_draw = height_draw
        self.human_heights_arg = None if human_heights is None else {
            g: ([float(x) for x in v] if isinstance(v, (list, tuple, np.ndarray)) else (None if v is None else float(v))) for g, v in human_heights.items()}
        base_heights = {g: v for g, v in (self.human_heights_arg or {}).items() if not isinstance(v, list)}
        if self.variants and (task != 'feeding' or reset_stream != 'philox'):
            raise NotImplementedError("%s: lists of heights are built for FeedingJaco's 'philox' resets; the PR2 tasks' host resets take one "
                                      "height per gender (the library's avr_human_variants_set serves all three rigid tasks)" % env_id)
        self.A, self.md = _scene(task, base_heights)
        self.human_heights = MC.human_heights(base_heights)
        self.task = self.md.task
        self.L = self.md.layout
        self.device_ik = self.task == ABI.TASK_FEEDING and reset_ik == 'device'
        self.device_dress_ik = self.task == ABI.TASK_DRESSING and reset_ik == 'device'
        self.device_search = self.task in (ABI.TASK_SCRATCH, ABI.TASK_BEDBATH) and reset_ik == 'device'
        self.scratch_attempts, self.scratch_iters = scratch_attempts, scratch_iters
        self.reset_stream = reset_stream
        self.device = device
        self.sim = _lib.Sim(self.md, self.n, device=device, seed=self.seed, env_offset=self.env_offset)
        self._variant_ctx = None
        if self.variants:
            # the variants' records are rebuilt (about 0.03 s each) and not cached: only their host link
            # origins stay, the device tables live in the handle
            recs = [MC.human_variant_records(ABI.SCENES[self.task], g, h, base=base_heights) for g, h in self.variants]
            self.sim.human_variants_set(recs)
            for R in recs:                  # (render: the base scene's hull planes serve every variant)
                RD.assert_variant_hulls(self.A, R['arrays'])
            self._variant_ctx = dict(slots={g: [2 + v for v, (vg, _) in enumerate(self.variants) if vg == g] for g in MC.GENDERS},
                                     pos={2 + v: R['human_pos'] for v, R in enumerate(recs)}, draw=height_draw)
        self.observation_space = Box(-1e9, 1e9, (self.L.OBS_DIM,))
        self.action_space = Box(-1.0, 1.0, (self.L.ACT_DIM,))
        self.obs_robot_len, self.obs_human_len = self.L.OBS_DIM, 0
        self.action_robot_len, self.action_human_len = self.L.ACT_DIM, 0
        self.genders = None                # setup(): fixed gender for every reset
        self.participant, self.policy_name = -1, ''
        self.hipbone_to_mouth_height = None   # setup(): kept, not modelled (see setup)
        self.episode = np.zeros(self.n, np.int64)
        # host mirror of the per-env iteration counters: the kernels' done is exactly
        # T_ITER >= max_steps (TimeLimit), so rollovers are known without reading the device
        self.iteration = np.zeros(self.n, np.int64)
        self.max_steps = int(self.md.params['max_episode_steps'])
        self._obs = np.zeros((self.n, self.L.OBS_DIM), np.float32)
        self._keepout = RS.keepout_box(self.A) if self.task == ABI.TASK_FEEDING else None
        if self.task == ABI.TASK_BEDBATH:          # the reset's arm settle, once per gender (device)
            from . import reset_bedbath as RBB
            RBB.settled_arms(self.A, self.md, device)
        self._prefetch = _Prefetch(self._inputs) if (prefetch and (self.device_ik or self.device_search or self.task == ABI.TASK_DRESSING)) else None
        self.last_ik_ok = None
        self.reset_timing = None

    # ------------------------------------------------------------------ setup hook
    def setup(self, gender, participant, policy_name, hipbone_to_mouth_height=None):
        """FeedingEnv.setup / ScratchItchEnv.setup (feeding.py:20-28): the evaluation harness fixes
        the participant's gender (every later reset uses it) and names the policy.

        hipbone_to_mouth_height is accepted and kept (`self.hipbone_to_mouth_height`) but, as in
        the reference's non-VR envs, does not shape the human: their reset overwrites it with the
        gender's default before building the world (feeding.py:173-174, scratch_itch.py:161,
        bed_bathing.py:187), so enjoy_vr.py's `env.setup(gender, participant, policy, 0.54)`
        (enjoy_vr.py:50,63) runs unchanged for both genders."""
        if gender not in ('male', 'female'):
            raise ValueError('gender must be male or female')
        self.hipbone_to_mouth_height = None if hipbone_to_mouth_height is None else float(hipbone_to_mouth_height)
        self.genders = gender
        self.participant, self.policy_name = int(participant), str(policy_name)
        if self._prefetch:
            self._prefetch.wait()
            self._prefetch.key = None      # draws prepared before setup() are for the old genders

    def _genders(self, idx):
        return None if self.genders is None else [self.genders] * len(idx)

    # ------------------------------------------------------------------ reset
    def _inputs(self, idx, episodes):
        """The host part of the masked envs' resets (everything before the device's part)."""
        ids = [self.env_offset + int(i) for i in idx]
        if self.task == ABI.TASK_DRESSING:
            from . import reset_dressing as RD
            P = RD.prepare_reset(self.A, self.md, self.seed, ids, genders=self._genders(idx), episodes=list(episodes))
            return P if self.device_dress_ik else RD.finish_reset(self.A, self.md, P)
        if self.task == ABI.TASK_BEDBATH:
            from . import reset_bedbath as RBB
            return RBB.prepare_reset(self.A, self.md, self.seed, ids, genders=self._genders(idx), episodes=list(episodes),
                                     attempts=self.scratch_attempts, device=self.device)
        if self.task == ABI.TASK_SCRATCH:
            from . import reset_scratch as RSS
            return RSS.prepare_reset(self.A, self.md, self.seed, ids, genders=self._genders(idx), impairment=self.impairment,
                                     episodes=list(episodes), attempts=self.scratch_attempts)
        out = RS.reset_inputs(self.A, self.md, self.seed, ids, genders=self._genders(idx),
                              impairment=self.impairment, episodes=list(episodes), stream=self.reset_stream, variants=self._variant_ctx)
        if self.new:        # the `new` human pose: waist and head draws, arms at 0 (redraw 0 of the clearance loop)
            RS.new_human_rows(self.A, out[0], self.seed, ids, list(episodes), [m['gender'] for m in out[4]], 0, self._variant_ctx)
        # + the self-contact screening's re-drawn target orientations (ik_random_restarts' step_sim)
        return out + (RS.ik_alt_orients(self.seed, ids, list(episodes), out[2].shape[1], self.reset_stream),)

    def _reset_rows(self, mask):
        idx = np.nonzero(mask)[0]
        if not len(idx):
            return
        self.iteration[idx] = 0
        eps = self.episode[idx].copy()
        S = np.zeros((self.n, self.L.STATE_WORDS), np.float32)
        frames = SETTLE_FRAMES[self.task]
        if self.device_ik:
            t0 = time.perf_counter()
            key = (tuple(idx.tolist()), tuple(eps.tolist()))
            got = self._prefetch.take(key) if self._prefetch else None
            Si, t7, init, _, meta, alt = got if got is not None else self._inputs(idx, eps)
            t1 = time.perf_counter()
            S[idx] = Si
            T = np.zeros((self.n, 7), np.float32)
            T[:, 6] = 1.0
            T[idx] = t7
            I = np.zeros((self.n,) + init.shape[1:], np.float32)
            I[idx] = init
            Al = np.zeros((self.n, init.shape[1], 4), np.float32)
            Al[..., 3] = 1.0
            Al[idx] = alt
            t2 = time.perf_counter()
            redraws = None
            if self.new:
                # the IK first (no settle yet), then the clearance loop on the host with the device
                # narrowphase at the IK pose, then the settle from the rows it leaves
                _, ok = self.sim.reset_ik(mask.astype(np.uint8), S, T, I, keepout8=self._keepout, frames=0, obs=self._obs, alt=Al)
                S = self.sim.get_state()
                rows = S[idx].astype(np.float64)
                ids = [self.env_offset + int(i) for i in idx]
                redraws, self.last_human_robot_distance = RS.new_redraw_loop(
                    self.A, rows, self.seed, ids, eps, [m['gender'] for m in meta],
                    lambda Sr, gl: RS.human_robot_distance(self.A, Sr, gl, self.sim.narrowphase), self._variant_ctx)
                S[idx] = rows
                self.sim.reset(mask.astype(np.uint8), S, frames, self._obs)
            else:
                _, ok = self.sim.reset_ik(mask.astype(np.uint8), S, T, I, keepout8=self._keepout, frames=frames, obs=self._obs, alt=Al)
            self.last_ik_ok = ok
            self.reset_timing = dict(inputs_s=t1 - t0, prefetched=got is not None, pack_s=t2 - t1, device_s=time.perf_counter() - t2)
            if redraws is not None:
                self.reset_timing['human_redraws'] = int(redraws.sum())
                self.reset_timing['human_redraws_max'] = int(redraws.max())
            if self._prefetch:           # speculate: the same envs end their next episode together
                self._prefetch.start((key[0], tuple((eps + 1).tolist())), idx, eps + 1)
            return
        ids = [self.env_offset + int(i) for i in idx]
        if self.task == ABI.TASK_DRESSING:
            # host draws (prefetched like the others' host parts), then the IK on the device
            # (avr_reset_ik) or, with reset_ik='host', the host IK and avr_reset
            t0 = time.perf_counter()
            key = (tuple(idx.tolist()), tuple(eps.tolist()))
            got = self._prefetch.take(key) if self._prefetch else None
            P = got if got is not None else self._inputs(idx, eps)
            t1 = time.perf_counter()
            if self._prefetch:
                self._prefetch.start((key[0], tuple((eps + 1).tolist())), idx, eps + 1)
            if self.device_dress_ik:
                Si, tpos, tquat, init, _ = P
                S[idx] = Si
                T = np.zeros((self.n, 7), np.float32)
                T[:, 6] = 1.0
                T[idx, :3], T[idx, 3:] = tpos, tquat
                I = np.zeros((self.n,) + init.shape[1:], np.float32)
                I[idx] = init
                _, ok = self.sim.reset_ik(mask.astype(np.uint8), S, T, I, iters=150, tol=0.01, frames=0, obs=self._obs)
                self.last_ik_ok = ok
            else:
                S[idx] = P[0]
                self.sim.reset(mask.astype(np.uint8), S, 0, self._obs)
            self.reset_timing = dict(host_s=t1 - t0, prefetched=got is not None, device_s=time.perf_counter() - t1)
            return
        if self.task in (ABI.TASK_SCRATCH, ABI.TASK_BEDBATH):
            # host part (prefetched on a background thread during the previous episode when the
            # same envs finish together), then the base-pose search on the device
            from . import reset_bedbath as RBB, reset_scratch as RSS
            t0 = time.perf_counter()
            key = (tuple(idx.tolist()), tuple(eps.tolist()))
            got = self._prefetch.take(key) if self._prefetch else None
            P = got if got is not None else self._inputs(idx, eps)
            t1 = time.perf_counter()
            fin = RBB.finish_reset if self.task == ABI.TASK_BEDBATH else RSS.finish_reset
            Si, _ = fin(self.A, self.md, P, self.scratch_iters, self.sim if self.device_search else None)
            t2 = time.perf_counter()
            if self._prefetch:
                self._prefetch.start((key[0], tuple((eps + 1).tolist())), idx, eps + 1)
            S[idx] = Si
            self.sim.reset(mask.astype(np.uint8), S, frames, self._obs)
            self.reset_timing = dict(inputs_s=t1 - t0, prefetched=got is not None, search_s=t2 - t1, device_s=time.perf_counter() - t2)
            return
        else:
            Si, _ = RS.batch_reset_states_fast(self.A, self.md, self.seed, ids, genders=self._genders(idx), impairment=self.impairment, episodes=eps,
                                               stream=self.reset_stream, self_contact=self.sim.robot_self_contact, variants=self._variant_ctx)
        S[idx] = Si
        self.sim.reset(mask.astype(np.uint8), S, frames, self._obs)

    def reset(self, mask=None):
        """Reset all envs (mask None) or the masked ones; returns obs (n_envs, obs_dim) float32."""
        mask = np.ones(self.n, bool) if mask is None else np.asarray(mask, bool)
        self._reset_rows(mask)
        return self._obs.copy()

    # ------------------------------------------------------------------ step
    def _info(self, inf):
        return {
            'total_force_on_human': inf[:, 0].copy(),
            'task_success': inf[:, 1].astype(np.int64),
            'action_robot_len': self.L.ACT_DIM, 'action_human_len': 0,
            'obs_robot_len': self.L.OBS_DIM, 'obs_human_len': 0,
        }

    def step(self, actions):
        """actions (n_envs, 7) -> obs, reward (n_envs,), done (n_envs,) bool, info dict of arrays.

        With auto_reset, finished envs are reset (next episode stream) and their final
        observation is returned in info['terminal_observation'] (vectorised-gym convention)."""
        a = np.ascontiguousarray(actions, np.float32).reshape(self.n, self.L.ACT_DIM)
        obs, rew, done, inf = self.sim.step(a)
        self.iteration += 1
        info = self._info(inf)
        self._obs[:] = obs
        if self.auto_reset and done.any():
            info['terminal_observation'] = obs.copy()
            self.episode[done] += 1
            self._reset_rows(done)
            obs = self._obs.copy()
        return obs, rew, done, info

    def observe(self):
        """Observation of the current state without stepping (what _get_obs returns right after
        p.restoreState, feeding.py:322-325)."""
        self._obs[:] = self.sim.settle(0)
        return self._obs.copy()

    def flags(self):
        """Per-env health flags (include/avr.h avr_get_flags), without copying the state.  Bits 0-4
        (_lib.FLAGS_FAULT_MASK) are faults, 0 there = healthy; bit 5 is informational (the env ran
        under the EPA budget, its state is finite)."""
        return self.sim.get_flags().astype(np.int64)

    def get_state(self):
        return self.sim.get_state()

    def proportions(self, S=None):
        """(genders, heights) of every env, from the proportions slot in its state row (S: state
        rows, default the current state): slot 0 / 1 are the handle's base male / female, 2 + v its
        height variant v."""
        S = self.get_state() if S is None else np.asarray(S)
        genders, heights = [], []
        for s in S[:, self.L.S_TASK + self.L.T_GENDER].astype(int):
            g, h = (('male', 'female')[s], None) if s < 2 else self.variants[s - 2]
            genders.append(g)
            heights.append(self.human_heights[g] if h is None else h)
        return genders, np.array(heights, float)

    def set_state(self, S):
        self.sim.set_state(S)
        self.iteration[:] = np.asarray(S)[:, self.L.S_TASK + self.L.T_ITER].astype(np.int64)

    # ------------------------------------------------------------------ views
    def _camera(self, camera, width, height):
        if self.task == ABI.TASK_DRESSING:
            raise NotImplementedError('render: not built for DressingJaco-v0')
        return (RD.default_camera(self.task) if camera is None else camera).resized(width, height)

    def render(self, mode='rgb_array', envs=None, camera=None, width=320, height=240, outputs=('rgb',)):
        """The envs as a camera sees their current state (include/avr.h avr_render_device): the
        collision shapes, ray-cast on the device -- gym's render(mode='rgb_array'), which the reference
        offers only as Bullet's GUI (env.py:613-620).  envs: the env indices (None: all; repeats
        allowed), camera: a render.Camera (None: the task's GUI camera, render.default_camera), always taken
        at width x height (the camera's own size is not used), outputs: some of 'rgb' [H, W, 3] uint8, 'depth' [H, W] float32 (metres along the
        ray, inf for a miss), 'id' [H, W] int32 (shape index, render.shape_table; -1 for a miss).
        Returns host arrays: one output alone, else a dict; with envs=None and one env [H, W, ...], the
        gym contract, else stacked [n, H, W, ...].  Reads the state only: stepping is not affected."""
        if mode != 'rgb_array':
            raise NotImplementedError("render: mode %r; only 'rgb_array' (there is no GUI)" % (mode,))
        cam = self._camera(camera, width, height)
        out = RD.render_host(self.sim, self.A, cam, None if envs is None else np.asarray(envs, np.int32).reshape(-1), tuple(outputs), device=self.device)
        if envs is None and self.n == 1:
            out = {k: v[0] for k, v in out.items()}
        return out[outputs[0]] if len(outputs) == 1 else out

    def close(self):
        if self._prefetch:
            self._prefetch.wait()
        self.sim.close()


class AVRTorchVecEnv(AVRVecEnv):
    """AVRVecEnv with torch device tensors: step(actions (n, 7) cuda float32) -> obs, reward, done,
    info as cuda tensors, written by the kernels directly (avr_step_device).  No per-step host
    traffic or synchronisation: whether a rollover is due follows from the host mirror of the
    iteration counters (done == T_ITER >= max_steps in the kernels), so launches of consecutive
    steps queue ahead of the GPU; a rollover step synchronises for the reset.

    reset_pool: None (default) keeps that behaviour.  reset_pool=m >= 1 moves the episode boundary onto
    the device (include/avr.h avr_rollover_*): the first reset() runs the reset path for episodes
    0 .. m-1 of every env (the same draws, IK and settle), collects the m * n_envs settled states and
    reset observations into a device-resident pool, leaves the envs in the last of them and switches
    the handle's rollover mode on.  From then on a finished env takes a pool state on the device: step()
    neither synchronises nor resets on the host, and rollout_policy runs any n steps across episode
    boundaries in one call.  Episodes then re-use the pool's initial states instead of drawing new ones
    (DESIGN.md).  pool_build_s holds the time the pool took to build.

    pool_world=(rank, world, group) (with reset_pool=m, one env per rank of a torch.distributed group, this
    one holding the global env ids [rank * n_envs, (rank + 1) * n_envs), i.e. env_offset = rank * n_envs):
    the ranks all-gather the pool rows they built before installing them, so every rank holds the same
    m * world * n_envs rows in the order one process of world * n_envs envs builds them (episode-major,
    global env within the episode), and a rollover picks the same state at any world size."""

    def __init__(self, *args, reset_pool=None, pool_world=None, **kw):
        if reset_pool is not None and (int(reset_pool) != reset_pool or int(reset_pool) < 1):
            raise ValueError('reset_pool must be None or an integer >= 1, not %r' % (reset_pool,))
        self.reset_pool = None if reset_pool is None else int(reset_pool)
        if pool_world is not None:
            if self.reset_pool is None:
                raise ValueError('pool_world needs reset_pool=m')
            rank, world, _ = pool_world
            if not 0 <= int(rank) < int(world):
                raise ValueError('pool_world: rank %r outside 0..%r' % (rank, int(world) - 1))
        self.pool_world = pool_world
        super().__init__(*args, **kw)
        if pool_world is not None and self.env_offset != int(pool_world[0]) * self.n:
            self.sim.close()
            raise ValueError('pool_world: rank %d of %d envs each needs env_offset=%d, not %d' % (pool_world[0], self.n, pool_world[0] * self.n, self.env_offset))
        if self.reset_pool and self.task == ABI.TASK_DRESSING:
            self.sim.close()
            raise NotImplementedError('reset_pool: the device rollover is not built for DressingJaco-v0')
        import torch
        self.torch = torch
        self.dev = torch.device('cuda', int(self.device))
        self.ext = torch.cuda.ExternalStream(self.sim.stream(), device=self.dev)
        n, L = self.n, self.L
        self.t_obs = torch.zeros(n, L.OBS_DIM, device=self.dev)
        self.t_rew = torch.zeros(n, device=self.dev)
        self.t_done = torch.zeros(n, dtype=torch.uint8, device=self.dev)
        self.t_info = torch.zeros(n, ABI.INFO_DIM, device=self.dev)
        self._cur = None                   # the current observation (what reset / step / rollout_policy last returned)
        self._roll = {}                    # rollout_policy's stacked output buffers, by rollout length
        self.policy_t = 0                  # rollout_policy's step index (keys the sampling noise; never reused)
        self._pool = None                  # reset_pool: (term_obs, term_value, episode) tensors over the handle's rollover rows
        self.pool_build_s = None

    def _wrap(self, ptr, shape, typestr):
        """A torch tensor over device memory the handle owns (no copy; valid until close())."""
        holder = type('_DevArray', (), {})()
        holder.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)
        return self.torch.as_tensor(holder, device=self.dev)

    def _build_pool(self):
        """The reset path for episodes 0 .. m-1 of every env into the handle's reset-state pool; the
        envs stay in the last of those resets.  The rollover rows are wrapped once."""
        t0 = time.perf_counter()
        every = np.ones(self.n, bool)
        S, O = [], []
        for ep in range(self.reset_pool):
            self.episode[:] = ep
            self._reset_rows(every)
            S.append(self.sim.get_state())
            O.append(self._obs.copy())
        S, O = np.stack(S), np.stack(O)                     # [m, n_envs, ...]
        if self.pool_world is not None and int(self.pool_world[1]) > 1:
            # every rank's rows, in global env order within each episode: the pool one process of all the envs builds
            from . import dist as D
            torch, group = self.torch, self.pool_world[2]
            S = D.gather_stacked(torch.from_numpy(S).to(self.dev), group).cpu().numpy()
            O = D.gather_stacked(torch.from_numpy(O).to(self.dev), group).cpu().numpy()
        self.sim.reset_pool_set(S.reshape(-1, S.shape[-1]), O.reshape(-1, O.shape[-1]))
        self.sim.rollover_enable(True)
        self.sim.rollover_set_episodes(self.episode)
        to, tv, ep = self.sim.rollover_buffers()
        self._pool = (self._wrap(to, (self.n, self.L.OBS_DIM), '<f4'), self._wrap(tv, (self.n,), '<f4'), self._wrap(ep, (self.n,), '<i4'))
        self.pool_build_s = time.perf_counter() - t0

    def _advance(self, n):
        """The host mirrors after n device steps with rollovers: done is T_ITER >= max_steps after the
        step's increment and a pool row restarts at T_ITER = 0, so iteration wraps at max_steps and
        episode increases there; no device read."""
        it = self.iteration
        first = np.maximum(self.max_steps - it, 1)          # steps to the env's first rollover
        rolled, rem = n >= first, n - first
        self.episode += np.where(rolled, 1 + rem // self.max_steps, 0)
        self.iteration = np.where(rolled, rem % self.max_steps, it + n)

    def reset(self, mask=None):
        if self.reset_pool and self._pool is None:
            self._build_pool()
            if mask is None:                # (the envs are in their last pool reset)
                self.t_obs.copy_(self.torch.from_numpy(self._obs))
                self._cur = self.t_obs.clone()
                return self.t_obs.clone()
        obs = super().reset(mask)
        self.t_obs.copy_(self.torch.from_numpy(obs))
        self._cur = self.t_obs.clone()
        return self.t_obs.clone()

    def step(self, actions):
        torch = self.torch
        a = actions.to(self.dev, torch.float32).contiguous()
        assert a.shape == (self.n, self.L.ACT_DIM)
        self.ext.wait_stream(torch.cuda.current_stream(self.dev))
        # (the kernels read `a` on the sim stream; torch's stream waits for that stream below, so the
        # caching allocator cannot hand `a`'s memory to later work before the step has read it)
        self.sim.step_device(a.data_ptr(), self.t_obs.data_ptr(), self.t_rew.data_ptr(), self.t_done.data_ptr(), self.t_info.data_ptr())
        torch.cuda.current_stream(self.dev).wait_stream(self.ext)
        if self._pool is not None:
            # the boundary on the device: finished envs take a pool state, t_obs rows become their reset
            # observations; the terminal ones are in the handle's rows (no host work, no synchronisation)
            self.sim.rollover_device(self.t_done.data_ptr(), self.t_obs.data_ptr())
            torch.cuda.current_stream(self.dev).wait_stream(self.ext)
            dh = self.iteration + 1 >= self.max_steps
            self._advance(1)
            obs, rew, done = self.t_obs.clone(), self.t_rew.clone(), self.t_done.bool()
            info = {'total_force_on_human': self.t_info[:, 0].clone(), 'task_success': self.t_info[:, 1].to(torch.int64),
                    'action_robot_len': self.L.ACT_DIM, 'action_human_len': 0, 'obs_robot_len': self.L.OBS_DIM, 'obs_human_len': 0}
            if dh.any():
                info['terminal_observation'] = torch.where(done[:, None], self._pool[0], obs)
            self._cur = obs
            return obs, rew, done, info
        self.iteration += 1
        obs, rew, done = self.t_obs.clone(), self.t_rew.clone(), self.t_done.bool()
        info = {'total_force_on_human': self.t_info[:, 0].clone(), 'task_success': self.t_info[:, 1].to(torch.int64),
                'action_robot_len': self.L.ACT_DIM, 'action_human_len': 0, 'obs_robot_len': self.L.OBS_DIM, 'obs_human_len': 0}
        if self.auto_reset:
            dh = self.iteration >= self.max_steps
            if dh.any():
                torch.cuda.current_stream(self.dev).synchronize()
                info['terminal_observation'] = obs
                self.episode[dh] += 1
                self._reset_rows(dh)
                m = torch.from_numpy(dh).to(self.dev)
                obs = torch.where(m[:, None], torch.from_numpy(self._obs).to(self.dev), obs)
        self._cur = obs
        return obs, rew, done, info

    def render_device(self, envs=None, camera=None, width=320, height=240, outputs=('rgb',)):
        """render() with device tensors and no host synchronisation: the images of the state as the
        steps queued so far leave it, in stream order with step() (the render waits for the caller's
        stream, the caller's stream for the render; a first call, or one with more envs than any before,
        allocates the handle's scratch, and an explicit env list is copied from host memory: include/avr.h
        avr_render_device).  Returns {name: cuda tensor [n, H, W, ...]} for the
        names in outputs ('rgb' uint8, 'depth' float32, 'id' int32)."""
        torch = self.torch
        cam = self._camera(camera, width, height)
        bad = [o for o in outputs if o not in ('depth', 'id', 'rgb')]
        if bad or not outputs:
            raise ValueError("render_device: outputs must name some of 'depth', 'id', 'rgb', not %r" % (tuple(outputs),))
        RD.install_planes(self.sim, self.A)
        ids = None if envs is None else np.asarray(envs, np.int32).reshape(-1)
        n = self.n if ids is None else len(ids)
        H, W = int(cam.height), int(cam.width)
        spec = {'depth': ((n, H, W), torch.float32), 'id': ((n, H, W), torch.int32), 'rgb': ((n, H, W, 3), torch.uint8)}
        buf = {k: torch.empty(spec[k][0], dtype=spec[k][1], device=self.dev) for k in outputs}
        self.ext.wait_stream(torch.cuda.current_stream(self.dev))
        self.sim.render_device(cam, ids, *[buf[k].data_ptr() if k in buf else None for k in ('depth', 'id', 'rgb')], n=n)
        torch.cuda.current_stream(self.dev).wait_stream(self.ext)
        return buf

    # ------------------------------------------------------------------ device-resident policy rollouts
    def set_policy(self, actor_critic, ob_rms):
        """Install (or, after an update of its weights, re-install) the policy rollout_policy runs:
        an ActorCritic and its ob_rms (None: no normalisation), packed by policy_eval.policy_desc.
        No graph is re-captured."""
        from .policy_eval import policy_desc
        self.sim.policy_set(policy_desc(actor_critic, ob_rms, self.L.OBS_DIM, self.L.ACT_DIM))

    def rollout_policy(self, actor_critic, ob_rms, n, deterministic=False):
        """n steps with the policy on the device, from the env's current observation, in one call
        with no host work per step (include/avr.h avr_rollout_policy_device).  actor_critic None:
        the policy installed by the last set_policy / rollout_policy call (pass it again after
        every weight update).  With auto_reset, n is capped so that the rollout ends at the
        TimeLimit at the latest, and finished episodes are rolled over after the call, as step does.

        Returns a dict of device tensors, stacked over the steps actually run, out['n']:
        obs [n+1, E, obs_dim] (slot 0 the current observation, slot k+1 the one after step k),
        act [n, E, act_dim], logp [n, E], value [n+1, E] (slot k = V(obs[k])), rew [n, E],
        done [n, E] uint8, info [n, E, 2] = {total_force_on_human, task_success}, and reset, the
        [E] bool mask of the envs rolled over after the call (None: none; obs[n] stays their
        terminal observation, the next rollout starts from their reset one).  The tensors are the
        env's own buffers, one set per rollout length: the next rollout of that length overwrites them.

        With a reset pool (reset_pool=m) n is not capped and nothing synchronises or resets on the
        host: an env with done[k] set starts its next episode at step k+1 from a pool state, obs[k+1]
        is its reset observation, reset is done.any(0) (a bool device tensor), and term_obs [E, obs_dim] /
        term_value [E] (views of the handle's rows) hold the terminal observation of each env's most
        recent rollover and its value."""
        torch = self.torch
        if self._cur is None:
            raise RuntimeError('rollout_policy: reset() the env first')
        if actor_critic is not None:
            self.set_policy(actor_critic, ob_rms)
        n = int(n)
        pooled = self._pool is not None
        if self.auto_reset and not pooled:
            n = min(n, int(self.max_steps - self.iteration.max()))
        if n < 1:
            raise ValueError('rollout_policy: n must be >= 1')
        E, L = self.n, self.L
        B = self._roll.get(n)
        if B is None:
            z = lambda *shape, **kw: torch.zeros(*shape, device=self.dev, **kw)
            B = self._roll[n] = dict(obs=z(n + 1, E, L.OBS_DIM), act=z(n, E, L.ACT_DIM), logp=z(n, E), value=z(n + 1, E), rew=z(n, E),
                                     done=z(n, E, dtype=torch.uint8), info=z(n, E, ABI.INFO_DIM))
        cur = self._cur.to(self.dev, torch.float32).contiguous()
        self.ext.wait_stream(torch.cuda.current_stream(self.dev))
        self.sim.rollout_policy_device(self.policy_t, n, cur.data_ptr(), deterministic,
                                       B['obs'].data_ptr(), B['act'].data_ptr(), B['logp'].data_ptr(), B['value'].data_ptr(),
                                       B['rew'].data_ptr(), B['done'].data_ptr(), B['info'].data_ptr())
        torch.cuda.current_stream(self.dev).wait_stream(self.ext)
        if pooled:
            # episode boundaries were crossed on the device: obs[k+1] of an env with done[k] is its reset
            # observation (act[k+1], logp[k+1] belong to it), the terminal one is in term_obs
            self._advance(n)
            self.policy_t += n
            self._cur = B['obs'][n].clone()
            return dict(B, n=n, reset=B['done'].bool().any(0), term_obs=self._pool[0], term_value=self._pool[1])
        self.iteration += n
        self.policy_t += n
        out = dict(B, n=n, reset=None)
        self._cur = B['obs'][n].clone()
        if self.auto_reset:
            dh = self.iteration >= self.max_steps
            if dh.any():
                torch.cuda.current_stream(self.dev).synchronize()
                self.episode[dh] += 1
                self._reset_rows(dh)
                m = torch.from_numpy(dh).to(self.dev)
                self._cur = torch.where(m[:, None], torch.from_numpy(self._obs).to(self.dev), self._cur)
                out['reset'] = m
        return out

    # ------------------------------------------------------------------ the PPO update on the device (avr/ppo.py)
    def compute_gae(self, out, gamma=0.99, lam=0.95, bootstrap=True):
        """Advantages and returns [n, E] of a rollout_policy result, on the device in stream order
        (include/avr.h avr_gae_device).  bootstrap: a done (always the TimeLimit here) bootstraps from
        V(terminal observation) -- needs a reset pool and n <= max_episode_steps; otherwise the return
        is cut at a done.  The tensors are the env's own, one pair per rollout length."""
        torch = self.torch
        n, E = out['rew'].shape
        B = self._roll.setdefault(('gae', n), {})
        if not B:
            B['adv'], B['ret'] = torch.zeros(n, E, device=self.dev), torch.zeros(n, E, device=self.dev)
        self.ext.wait_stream(torch.cuda.current_stream(self.dev))
        self.sim.gae_device(n, gamma, lam, bootstrap, out['rew'].data_ptr(), out['done'].data_ptr(), out['value'].data_ptr(),
                            B['adv'].data_ptr(), B['ret'].data_ptr())
        torch.cuda.current_stream(self.dev).wait_stream(self.ext)
        return B['adv'], B['ret']

    def ppo_reset(self):
        """Zero the optimiser state of ppo_update (Adam's moments and step count; include/avr.h
        avr_ppo_reset).  set_policy does not do it: call this after installing a different network,
        whose weights the old moments do not belong to."""
        from . import _lib
        self.sim.ppo_reset()
        if getattr(self, '_ppo_stats', None) is None:
            self._ppo_stats = self._wrap(self.sim.ppo_buffers()[3], (_lib.PPO_STATS_ROWS, _lib.PPO_STAT_WORDS), '<f4')

    def ppo_update(self, out, adv, ret, params, epochs, n_minibatch, generator=None):
        """epochs x n_minibatch PPO minibatch steps on the installed policy's weight block, in place and
        in stream order (include/avr.h avr_ppo_update_device); the next rollout_policy(None, None, n)
        runs the new weights.  out: a rollout_policy result, adv / ret: compute_gae's, params: a dict
        with avr/ppo.py DEFAULTS' loss and Adam keys.  The minibatch permutations are torch.randperm
        draws on the device (generator: a torch.Generator on it).  The optimiser state is zeroed by
        ppo_reset() -- run for the caller before the env's first update only; set_policy keeps it, so
        call ppo_reset() after installing a different network.  Returns the statistics rows [epochs * n_minibatch, 6]
        (columns _lib.PPO_STATS), a device tensor; at most PPO_STATS_ROWS rows are kept."""
        from . import _lib
        torch = self.torch
        n, E = out['rew'].shape
        N = n * E
        if getattr(self, '_ppo_stats', None) is None:
            self.ppo_reset()
        perm = torch.stack([torch.randperm(N, device=self.dev, generator=generator) for _ in range(int(epochs))]).to(torch.int32).contiguous()
        batch = self.sim.ppo_batch(n, E, obs=out['obs'].data_ptr(), act=out['act'].data_ptr(), logp=out['logp'].data_ptr(),
                                   value=out['value'].data_ptr(), adv=adv.data_ptr(), ret=ret.data_ptr())
        self.ext.wait_stream(torch.cuda.current_stream(self.dev))
        self.sim.ppo_update_device(batch, self.sim.ppo_params(params), epochs, n_minibatch, perm.data_ptr())
        torch.cuda.current_stream(self.dev).wait_stream(self.ext)
        rows = min(int(epochs) * int(n_minibatch), _lib.PPO_STATS_ROWS)
        return self._ppo_stats[:rows, :len(_lib.PPO_STATS)].clone()

    # ------------------------------------------------------------------ reward normalisation and episode statistics
    def normalize_rewards(self, out, gamma, clip_rew=10.0, eps=1e-8, update=True):
        """VecNormalize's reward half on a rollout_policy result, on the device in stream order
        (include/avr.h avr_reward_norm_device): out['rew'] / sqrt(var + eps) clipped to +-clip_rew, var the
        running variance of the discounted return, which the handle carries across rollouts (reset by
        train_stats_reset).  update False: eval mode, the carried state is only read.  out['rew'] itself
        is left as it is; the returned [n, E] tensor is the env's own, one per rollout length."""
        torch = self.torch
        n, E = out['rew'].shape
        B = self._roll.setdefault(('rew_norm', n), {})
        if not B:
            B['rew'] = torch.zeros(n, E, device=self.dev)
        self.ext.wait_stream(torch.cuda.current_stream(self.dev))
        self.sim.reward_norm_device(n, gamma, clip_rew, eps, update, out['rew'].data_ptr(), out['done'].data_ptr(), B['rew'].data_ptr())
        torch.cuda.current_stream(self.dev).wait_stream(self.ext)
        return B['rew']

    def _train_stats_row(self):
        from . import _lib
        if getattr(self, '_ep_row', None) is None:
            self._ep_row = self._wrap(self.sim.train_stats_buffers()[3], (_lib.EPSTAT_WORDS,), '<f8')
        return self._ep_row

    def episode_stats(self, out):
        """Advance the handle's per-env episode accumulators over a rollout_policy result (its raw rew, done
        and info) in stream order and return the aggregate over the episodes that ended in it: a cloned
        device float64 row with the columns _lib.EPISODE_STATS (include/avr.h avr_episode_stats_device;
        PPOTrainer.episode_summary turns it into means).  Nothing is synchronised."""
        torch = self.torch
        n = out['rew'].shape[0]
        row = self._train_stats_row()
        self.ext.wait_stream(torch.cuda.current_stream(self.dev))
        self.sim.episode_stats_device(n, out['rew'].data_ptr(), out['done'].data_ptr(), out['info'].data_ptr())
        torch.cuda.current_stream(self.dev).wait_stream(self.ext)
        return row.clone()

    def train_stats_reset(self):
        """Zero the state normalize_rewards and episode_stats carry across rollouts: the discounted returns,
        their running moments (back to mean 0, var 1, count 1e-4) and the episode accumulators."""
        torch = self.torch
        self.ext.wait_stream(torch.cuda.current_stream(self.dev))
        self.sim.train_stats_reset()
        torch.cuda.current_stream(self.dev).wait_stream(self.ext)

    def close(self):
        self.torch.cuda.synchronize(self.dev)
        super().close()


class AVREnv:
    """Single-env view with the reference's gym.Env signatures."""

    def __init__(self, env_id='FeedingJaco-v0', device=0, seed=1001, impairment='random'):
        self.v = AVRVecEnv(env_id, 1, device=device, seed=seed, auto_reset=False, impairment=impairment, prefetch=False)
        self.observation_space = self.v.observation_space
        self.action_space = self.v.action_space

    def seed(self, seed=1001):
        self.v.seed = int(seed)
        return [seed]

    def reset(self):
        return self.v.reset()[0].astype(np.float64)

    def step(self, action):
        obs, rew, done, info = self.v.step(np.asarray(action, np.float32)[None])
        i = {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in info.items()}
        i['task_success'] = int(i['task_success'])
        i['total_force_on_human'] = float(i['total_force_on_human'])
        return obs[0].astype(np.float64), float(rew[0]), bool(done[0]), i

    def render(self, mode='rgb_array', **kw):
        """gym's render(mode='rgb_array'): [height, width, 3] uint8 (AVRVecEnv.render's keywords)."""
        return self.v.render(mode=mode, **kw)

    def close(self):
        self.v.close()


def make(env_id, **kw):
    """gym.make replacement: AVREnv for one env, AVRVecEnv when n_envs is given (AVRTorchVecEnv
    with torch=True)."""
    if kw.pop('torch', False):
        return AVRTorchVecEnv(env_id, **kw)
    if 'n_envs' in kw:
        return AVRVecEnv(env_id, **kw)
    return AVREnv(env_id, **kw)
