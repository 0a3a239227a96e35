"""ctypes binding of libavr.so (include/avr.h) -- the product path.

The library is built in-tree (`python -m avr.build` or `__graft_entry__.build()`) for gfx950.
There is no fallback: if the shared object or a GPU is missing, the calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import _abi as ABI

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('AVR_LIB') or os.path.join(HERE, 'libavr.so')   # AVR_LIB: experiment builds

EXPORTS = [
    'avr_create', 'avr_destroy', 'avr_set_state', 'avr_get_state', 'avr_set_state_masked', 'avr_settle',
    'avr_step', 'avr_step_device', 'avr_step_random_device', 'avr_rollout_random_device', 'avr_random_actions_device', 'avr_sync',
    'avr_stream', 'avr_state_device_ptr', 'avr_n_envs', 'avr_env_groups', 'avr_dyn_split', 'avr_pairs_flat', 'avr_np_hot', 'avr_coop_wsup', 'avr_state_words', 'avr_abi_version',
    'avr_kernel_info', 'avr_last_error', 'avr_substep', 'avr_reset', 'avr_profile_kernels', 'avr_kernel_times',
    'avr_hull_support_table', 'avr_task', 'avr_task_state_words', 'avr_task_obs_dim', 'avr_task_act_dim', 'avr_n_dof',
    'avr_get_q', 'avr_get_link_pose', 'avr_get_contact_summary', 'avr_get_flags', 'avr_reset_ik', 'avr_base_search',
    'avr_graph_captures', 'avr_robot_self_contact', 'avr_narrowphase_query', 'avr_bb_closest_query',
    'avr_policy_set', 'avr_policy_act_device', 'avr_rollout_policy_device',
    'avr_reset_pool_set', 'avr_rollover_enable', 'avr_rollover_device', 'avr_rollover_buffers', 'avr_rollover_set_episodes',
    'avr_human_variants_set', 'avr_human_variants', 'avr_human_variant_info', 'avr_narrowphase_query_slots',
    'avr_gae_device', 'avr_ppo_reset', 'avr_ppo_grad_device', 'avr_ppo_adam_device', 'avr_ppo_update_device', 'avr_ppo_buffers',
    'avr_ppo_words', 'avr_policy_block', 'avr_policy_get', 'avr_policy_obs_norm_device',
    'avr_ppo_advstat_device', 'avr_ppo_grad_segment_device', 'avr_ppo_combine_device',
    'avr_reward_norm_device', 'avr_episode_stats_device', 'avr_train_stats_reset', 'avr_train_stats_buffers',
    'avr_n_bodies', 'avr_get_body_poses', 'avr_render_set_planes', 'avr_render_device', 'avr_render_tile_stats', 'avr_render_kernel_info',
]
RENDER_TILE = 8              # csrc/avr_render.hip RD_TILE: a wavefront traces an 8 x 8 pixel tile
PPO_STAT_WORDS, PPO_STATS_ROWS = 8, 256      # include/avr.h AVR_PPO_STAT_WORDS, AVR_PPO_STATS_ROWS
PPO_STATS = ('policy_loss', 'value_loss', 'entropy', 'approx_kl', 'clip_frac', 'grad_norm')   # a statistics row's first words
PPO_SEGMENTS = 8             # include/avr.h AVR_PPO_SEGMENTS: segments of a minibatch, whatever the rank count
PPO_SEG_WORDS = 13144 + PPO_STAT_WORDS       # include/avr.h AVR_PPO_SEG_WORDS: the weight block's words, then a statistics row's
# include/avr.h AVR_EPSTAT_WORDS: the columns of avr_episode_stats_device's aggregate row (float64)
EPISODE_STATS = ('episodes', 'ret_sum', 'ret_sumsq', 'ret_min', 'ret_max', 'len_sum', 'success_sum', 'force_mean_sum', 'steps', 'rew_sum')
EPSTAT_WORDS = len(EPISODE_STATS)
# include/avr.h AVR_EPENV_*: the per-env episode rows (4-byte words) and each row's dtype
EPISODE_ENV_ROWS = (('ep_ret', '<f4'), ('ep_len', '<i4'), ('ep_force', '<f4'), ('last_ret', '<f4'), ('last_len', '<i4'), ('last_success', '<f4'),
                    ('n_finished', '<i4'))
TS_RED_THREADS = 256         # csrc/avr_trainstats.hip: threads of a reduction block (a thread folds envs t, t + 256, ...)
MAX_HUMAN_VARIANTS = 64     # include/avr.h AVR_MAX_HUMAN_VARIANTS
FLAGS_FAULT_MASK = 0x1f      # include/avr.h AVR_FLAGS_FAULT_MASK: bits 0-4; bit 5 (EPA budget) is informational


# avr_config.flags: no bit is defined (include/avr.h); avr_create rejects any set bit


class avr_config(C.Structure):
    _fields_ = [('n_envs', C.c_int32), ('device', C.c_int32), ('env_offset', C.c_int32), ('flags', C.c_int32),
                ('seed', C.c_uint64)]


class avr_policy_desc(C.Structure):
    """include/avr.h avr_policy_desc: host float32 arrays, matrices row-major [out][in]."""
    ARRAYS = ('ob_mean', 'ob_var', 'a_w1', 'a_b1', 'a_w2', 'a_b2', 'mu_w', 'mu_b', 'logstd', 'c_w1', 'c_b1', 'c_w2', 'c_b2', 'c_w3', 'c_b3')
    _fields_ = [('obs_dim', C.c_int32), ('act_dim', C.c_int32), ('hidden', C.c_int32), ('n_layers', C.c_int32),
                ('clip_obs', C.c_float), ('eps', C.c_float)] + [(k, C.c_void_p) for k in ARRAYS]


class avr_ppo_batch(C.Structure):
    """include/avr.h avr_ppo_batch: device pointers of a flattened [n][E] batch."""
    ARRAYS = ('obs', 'act', 'logp', 'value', 'adv', 'ret')
    _fields_ = [('n', C.c_int32), ('E', C.c_int32)] + [(k, C.c_void_p) for k in ARRAYS]


class avr_ppo_params(C.Structure):
    """include/avr.h avr_ppo_params."""
    FLOATS = ('clip', 'vf_coef', 'ent_coef', 'max_grad_norm', 'lr', 'beta1', 'beta2', 'eps')
    _fields_ = [(k, C.c_float) for k in FLOATS] + [('norm_adv', C.c_int32), ('clip_value', C.c_int32)]


class avr_policy_out(C.Structure):
    """include/avr.h avr_policy_out: host float32 arrays avr_policy_get fills, matrices [out][in]."""
    ARRAYS = avr_policy_desc.ARRAYS
    _fields_ = [('hidden', C.c_int32), ('has_ob_rms', C.c_int32), ('has_critic', C.c_int32), ('clip_obs', C.c_float), ('eps', C.c_float)] + [
        (k, C.c_void_p) for k in ARRAYS]


class avr_human_variant(C.Structure):
    """include/avr.h avr_human_variant: one height variant's float32 records (host arrays)."""
    ARRAYS = ('shape_pose', 'shape_param', 'shape_aabb', 'body_aabb', 'body_threshold', 'hc_jpos', 'hc_inertia', 'bb_targets')
    _fields_ = [('gender', C.c_int32), ('height', C.c_float), ('n_gshapes', C.c_int32), ('n_hbodies', C.c_int32)] + [(k, C.c_void_p) for k in ARRAYS]


class avr_camera(C.Structure):
    """include/avr.h avr_camera."""
    _fields_ = [('eye', C.c_float * 3), ('target', C.c_float * 3), ('up', C.c_float * 3), ('fov_y_deg', C.c_float), ('near', C.c_float),
                ('far', C.c_float), ('width', C.c_int32), ('height', C.c_int32), ('body', C.c_int32), ('reserved', C.c_int32 * 3)]


_LIB = None


def load(path=LIB_PATH):
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(path):
        raise RuntimeError('libavr.so not built (%s); run __graft_entry__.build()' % path)
    # One HIP runtime per process: if torch is importable, let it load its libamdhip64 first so
    # libavr binds to the same runtime (device pointers from torch tensors stay valid here).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.avr_create.argtypes = [C.POINTER(avr_config), vp, C.POINTER(vp)]
    if hasattr(lib, 'avr_hull_support_table'):      # (absent in experiment builds of older trees)
        lib.avr_hull_support_table.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int32]
        lib.avr_hull_support_table.restype = C.c_int32
    lib.avr_destroy.argtypes = [vp]
    lib.avr_set_state.argtypes = [vp, vp]
    lib.avr_get_state.argtypes = [vp, vp]
    lib.avr_set_state_masked.argtypes = [vp, vp, vp]
    lib.avr_settle.argtypes = [vp, C.c_int32, vp]
    lib.avr_step.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.avr_step_device.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.avr_step_random_device.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
    lib.avr_rollout_random_device.argtypes = [vp, C.c_int64, C.c_int32, vp, vp, vp, vp, C.c_int32]
    lib.avr_random_actions_device.argtypes = [vp, C.c_int64, vp]
    if hasattr(lib, 'avr_policy_set'):              # (absent in experiment builds of older trees)
        lib.avr_policy_set.argtypes = [vp, C.POINTER(avr_policy_desc)]
        lib.avr_policy_act_device.argtypes = [vp, C.c_int64, vp, C.c_int32, vp, vp, vp]
        lib.avr_rollout_policy_device.argtypes = [vp, C.c_int64, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, 'avr_reset_pool_set'):          # (absent in experiment builds of older trees)
        lib.avr_reset_pool_set.argtypes = [vp, C.c_int32, vp, vp]
        lib.avr_rollover_enable.argtypes = [vp, C.c_int32]
        lib.avr_rollover_device.argtypes = [vp, vp, vp]
        lib.avr_rollover_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        lib.avr_rollover_set_episodes.argtypes = [vp, vp]
    if hasattr(lib, 'avr_human_variants_set'):      # (absent in experiment builds of older trees)
        lib.avr_human_variants_set.argtypes = [vp, C.c_int32, vp]
        lib.avr_human_variants.argtypes = [vp]
        lib.avr_human_variants.restype = C.c_int32
        lib.avr_human_variant_info.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        lib.avr_narrowphase_query_slots.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_float, vp]
    if hasattr(lib, 'avr_ppo_reset'):               # (absent in experiment builds of older trees)
        lib.avr_gae_device.argtypes = [vp, C.c_int32, C.c_float, C.c_float, C.c_int32, vp, vp, vp, vp, vp]
        lib.avr_ppo_reset.argtypes = [vp]
        lib.avr_ppo_grad_device.argtypes = [vp, C.POINTER(avr_ppo_batch), C.POINTER(avr_ppo_params), C.c_int32, C.c_int32, vp]
        lib.avr_ppo_adam_device.argtypes = [vp, C.POINTER(avr_ppo_params)]
        lib.avr_ppo_update_device.argtypes = [vp, C.POINTER(avr_ppo_batch), C.POINTER(avr_ppo_params), C.c_int32, C.c_int32, vp]
        lib.avr_ppo_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        lib.avr_ppo_words.restype = C.c_int32
        lib.avr_policy_block.argtypes = [vp]
        lib.avr_policy_block.restype = vp
        lib.avr_policy_get.argtypes = [vp, C.POINTER(avr_policy_out)]
        lib.avr_policy_obs_norm_device.argtypes = [vp, vp, vp]
    if hasattr(lib, 'avr_ppo_combine_device'):      # (absent in experiment builds of older trees)
        lib.avr_ppo_advstat_device.argtypes = [vp, C.POINTER(avr_ppo_batch)]
        lib.avr_ppo_grad_segment_device.argtypes = [vp, C.POINTER(avr_ppo_batch), C.POINTER(avr_ppo_params), C.c_int32, C.c_int32, vp, C.c_int32, vp]
        lib.avr_ppo_combine_device.argtypes = [vp, C.POINTER(avr_ppo_params), vp]
    if hasattr(lib, 'avr_train_stats_reset'):       # (absent in experiment builds of older trees)
        lib.avr_reward_norm_device.argtypes = [vp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, vp, vp, vp]
        lib.avr_episode_stats_device.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
        lib.avr_train_stats_reset.argtypes = [vp]
        lib.avr_train_stats_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    if hasattr(lib, 'avr_render_device'):           # (absent in experiment builds of older trees)
        lib.avr_n_bodies.argtypes = [vp]
        lib.avr_n_bodies.restype = C.c_int32
        lib.avr_get_body_poses.argtypes = [vp, vp]
        lib.avr_render_set_planes.argtypes = [vp, C.c_int32, vp, vp]
        lib.avr_render_device.argtypes = [vp, C.POINTER(avr_camera), C.c_int32, vp, vp, vp, vp]
        lib.avr_render_tile_stats.argtypes = [vp, C.POINTER(avr_camera), C.c_int32, vp, vp]
        lib.avr_render_kernel_info.argtypes = [vp, vp]
    lib.avr_sync.argtypes = [vp]
    lib.avr_stream.argtypes = [vp]
    lib.avr_stream.restype = vp
    lib.avr_state_device_ptr.argtypes = [vp]
    lib.avr_state_device_ptr.restype = vp
    lib.avr_n_envs.argtypes = [vp]
    lib.avr_env_groups.argtypes = [vp]
    lib.avr_env_groups.restype = C.c_int32
    lib.avr_dyn_split.argtypes = [vp]
    lib.avr_dyn_split.restype = C.c_int32
    lib.avr_pairs_flat.argtypes = [vp]
    lib.avr_pairs_flat.restype = C.c_int32
    lib.avr_np_hot.argtypes = [vp]
    lib.avr_np_hot.restype = C.c_int32
    lib.avr_coop_wsup.argtypes = [vp]
    lib.avr_coop_wsup.restype = C.c_int32
    lib.avr_graph_captures.argtypes = [vp]
    lib.avr_graph_captures.restype = C.c_int64
    lib.avr_state_words.restype = C.c_int32
    lib.avr_abi_version.restype = C.c_int32
    lib.avr_kernel_info.argtypes = [vp, vp]
    lib.avr_last_error.argtypes = [vp]
    lib.avr_last_error.restype = C.c_char_p
    lib.avr_substep.argtypes = [vp, C.c_float]
    lib.avr_reset.argtypes = [vp, vp, vp, C.c_int32, vp]
    lib.avr_profile_kernels.argtypes = [vp, C.c_int32]
    lib.avr_kernel_times.argtypes = [vp, vp, vp]
    lib.avr_task.argtypes = [vp]
    lib.avr_n_dof.argtypes = [vp]
    for f in ('avr_task_state_words', 'avr_task_obs_dim', 'avr_task_act_dim'):
        getattr(lib, f).argtypes = [C.c_int32]
        getattr(lib, f).restype = C.c_int32
    lib.avr_get_q.argtypes = [vp, vp, vp]
    lib.avr_get_link_pose.argtypes = [vp, C.c_int32, vp]
    lib.avr_get_contact_summary.argtypes = [vp, vp]
    lib.avr_get_flags.argtypes = [vp, vp]
    lib.avr_reset_ik.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_float, vp, C.c_int32, vp, vp]
    lib.avr_robot_self_contact.argtypes = [vp, C.c_int32, vp, vp]
    lib.avr_narrowphase_query.argtypes = [vp, C.c_int32, vp, vp, C.c_float, vp]
    if hasattr(lib, 'avr_bb_closest_query'):        # (absent in experiment builds of older trees)
        lib.avr_bb_closest_query.argtypes = [vp, C.c_int32, vp]
    lib.avr_base_search.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, C.c_float, vp, vp, vp, vp]
    if lib.avr_abi_version() != ABI.ABI_VERSION or any(
            lib.avr_task_state_words(t) != L.STATE_WORDS or lib.avr_task_obs_dim(t) != L.OBS_DIM or lib.avr_task_act_dim(t) != L.ACT_DIM
            for t, L in ABI.LAYOUTS.items()):
        raise RuntimeError('%s: ABI %d / state layouts differ from this package (ABI %d); rebuild'
                           % (path, lib.avr_abi_version(), ABI.ABI_VERSION))
    _LIB = lib
    return lib


class Sim:
    """One libavr handle = one GPU, n_envs environments."""

    def __init__(self, md, n_envs, device=0, seed=1001, env_offset=0, flags=0):
        """flags: avr_config.flags, must be 0 (include/avr.h)."""
        self.lib = load()
        self.md = md
        self.n = int(n_envs)
        self.kernel_kinds = ('avr_take_step_kernel', 'avr_substep_a_kernel', 'avr_substep_b4_kernel', 'avr_task_kernel',
                             'avr_substep_pairs_kernel', 'avr_narrowphase_kernel', 'avr_coop_kernel')
        cfg = avr_config(n_envs=self.n, device=device, env_offset=env_offset, flags=int(flags), seed=seed)
        h = C.c_void_p()
        rc = self.lib.avr_create(C.byref(cfg), C.cast(md.ptr(), C.c_void_p), C.byref(h))
        self.h = h
        if rc:
            msg = self.lib.avr_last_error(h).decode() if h.value else 'avr_create failed'
            if h.value:
                self.lib.avr_destroy(h)
                self.h = None
            raise RuntimeError('avr_create failed (%d): %s' % (rc, msg))
        self.task = int(self.lib.avr_task(h))
        self.L = ABI.LAYOUTS[self.task]
        if self.task == ABI.TASK_DRESSING:      # one kernel per step, timed in kind slot 2 (avr_dressing.hip)
            self.kernel_kinds = ('-', '-', 'avr_dress_step_kernel', '-', '-', '-', '-')
        self.words = self.lib.avr_task_state_words(self.task)
        self.obs_dim, self.act_dim = self.L.OBS_DIM, self.L.ACT_DIM

    def _chk(self, rc):
        if rc:
            raise RuntimeError(self.lib.avr_last_error(self.h).decode())

    def close(self):
        if getattr(self, 'h', None):
            self.lib.avr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, S):
        S = np.ascontiguousarray(S, np.float32).reshape(self.n, self.words)
        self._chk(self.lib.avr_set_state(self.h, S.ctypes.data))

    def set_state_masked(self, mask, S):
        S = np.ascontiguousarray(S, np.float32).reshape(self.n, self.words)
        mask = np.ascontiguousarray(mask, np.uint8)
        self._chk(self.lib.avr_set_state_masked(self.h, mask.ctypes.data, S.ctypes.data))

    def get_state(self):
        S = np.zeros((self.n, self.words), np.float32)
        self._chk(self.lib.avr_get_state(self.h, S.ctypes.data))
        return S

    def settle(self, frames=100):
        obs = np.zeros((self.n, self.obs_dim), np.float32)
        self._chk(self.lib.avr_settle(self.h, frames, obs.ctypes.data))
        return obs

    def reset(self, mask, S, frames=100, obs=None):
        """Masked episode reset (include/avr.h avr_reset): rows of S for mask!=0, settle, obs."""
        S = np.ascontiguousarray(S, np.float32).reshape(self.n, self.words)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(self.n)
        if obs is None:
            obs = np.zeros((self.n, self.obs_dim), np.float32)
        assert obs.dtype == np.float32 and obs.flags.c_contiguous and obs.shape == (self.n, self.obs_dim)
        self._chk(self.lib.avr_reset(self.h, None if m is None else m.ctypes.data, S.ctypes.data, int(frames), obs.ctypes.data))
        return obs

    def reset_ik(self, mask, S, target7, init, iters=80, tol=0.01, keepout8=None, frames=100, obs=None, alt=None):
        """Masked reset with the IK on the device (include/avr.h avr_reset_ik): S rows without the
        arm joints, target7 (n_envs, 7), init (n_envs, restarts, n_arm) restart draws, alt
        (n_envs, restarts, 4) the self-contact screening's re-drawn orientations (None: no
        screening).  Returns (obs, ok)."""
        S = np.ascontiguousarray(S, np.float32).reshape(self.n, self.words)
        t = np.ascontiguousarray(target7, np.float32).reshape(self.n, 7)
        init = np.ascontiguousarray(init, np.float32)
        assert init.ndim == 3 and init.shape[0] == self.n
        if alt is not None:
            alt = np.ascontiguousarray(alt, np.float32)
            assert alt.shape == (self.n, init.shape[1], 4)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(self.n)
        box = None if keepout8 is None else np.ascontiguousarray(keepout8, np.float32).reshape(8)
        if obs is None:
            obs = np.zeros((self.n, self.obs_dim), np.float32)
        assert obs.dtype == np.float32 and obs.flags.c_contiguous and obs.shape == (self.n, self.obs_dim)
        ok = np.zeros(self.n, np.uint8)
        self._chk(self.lib.avr_reset_ik(self.h, None if m is None else m.ctypes.data, S.ctypes.data, t.ctypes.data, init.ctypes.data,
                                        None if alt is None else alt.ctypes.data, int(init.shape[1]), int(iters), float(tol), None if box is None else box.ctypes.data, int(frames),
                                        obs.ctypes.data, ok.ctypes.data))
        return obs, ok.astype(bool)

    def robot_self_contact(self, Q):
        """Touching robot shape pairs at each row of Q (n, n_dof()) -- avr_get_q's layout, or just
        the robot DoFs (the human chain's then 0) -- (include/avr.h avr_robot_self_contact:
        p.getContactPoints(robot, robot) after a reset restart)."""
        Q = np.asarray(Q, np.float32)
        nd = self.n_dof()
        assert Q.ndim == 2 and Q.shape[1] <= nd
        q = np.zeros((len(Q), nd), np.float32)
        q[:, :Q.shape[1]] = Q
        out = np.zeros(len(q), np.int32)
        self._chk(self.lib.avr_robot_self_contact(self.h, int(len(q)), q.ctypes.data, out.ctypes.data))
        return out

    def narrowphase(self, pairs, poses14, thr=0.02, slots=None):
        """The step's narrowphase per (sa, sb) row of pairs at body poses poses14 (n, 14)
        (include/avr.h avr_narrowphase_query): (n, 8) {rc, normal on B, point on B, distance}.
        slots (n,): each query's proportions slot, its shapes from that height variant's tables
        (avr_narrowphase_query_slots)."""
        p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        x = np.ascontiguousarray(poses14, np.float32).reshape(len(p), 14)
        out = np.zeros((len(p), 8), np.float32)
        if slots is None:
            self._chk(self.lib.avr_narrowphase_query(self.h, int(len(p)), p.ctypes.data, x.ctypes.data, float(thr), out.ctypes.data))
        else:
            sl = np.ascontiguousarray(slots, np.int32).reshape(len(p))
            self._chk(self.lib.avr_narrowphase_query_slots(self.h, int(len(p)), p.ctypes.data, x.ctypes.data, sl.ctypes.data, float(thr), out.ctypes.data))
        return out

    def bb_closest_query(self, cap=-1):
        """BedBathing's closest tool-human distance of every env's current state, by the step's code
        (include/avr.h avr_bb_closest_query): (n_envs, 4) {final minimum, queued stalled pairs,
        minimum before their rerun, stalled pairs past the queue's capacity}.  cap: the queue's
        capacity for this call (negative: the step's)."""
        out = np.zeros((self.n, 4), np.float32)
        self._chk(self.lib.avr_bb_closest_query(self.h, int(cap), out.ctypes.data))
        return out

    def base_search(self, base7, rest, tstart, goals, iters=200, tol=0.03, per_attempt=False):
        """PR2 base-pose search on the device (include/avr.h avr_base_search): base7 (n, attempts, 7),
        rest (n, attempts, n_arm), tstart (n, 3), goals (n, 3, 3).  Returns (best (n,) attempt index,
        ok (n,) bool, q_arm (n, n_arm)[, res (n, attempts, 4) when per_attempt])."""
        b = np.ascontiguousarray(base7, np.float32)
        assert b.ndim == 3 and b.shape[2] == 7
        n, att = b.shape[:2]
        r = np.ascontiguousarray(rest, np.float32)
        na = r.shape[2]
        assert r.shape[:2] == (n, att)
        t = np.ascontiguousarray(tstart, np.float32).reshape(n, 3)
        g = np.ascontiguousarray(goals, np.float32).reshape(n, 9)
        best = np.zeros(n, np.int32)
        ok = np.zeros(n, np.uint8)
        q = np.zeros((n, na), np.float32)
        res = np.zeros((n, att, 4), np.float32) if per_attempt else None
        self._chk(self.lib.avr_base_search(self.h, int(n), int(att), b.ctypes.data, r.ctypes.data, t.ctypes.data, g.ctypes.data, int(iters),
                                           float(tol), best.ctypes.data, ok.ctypes.data, q.ctypes.data, None if res is None else res.ctypes.data))
        return (best, ok.astype(bool), q) + ((res,) if per_attempt else ())

    def substep(self, dt):
        self._chk(self.lib.avr_substep(self.h, dt))

    def step(self, act):
        act = np.ascontiguousarray(act, np.float32).reshape(self.n, self.act_dim)
        obs = np.zeros((self.n, self.obs_dim), np.float32)
        rew = np.zeros(self.n, np.float32)
        done = np.zeros(self.n, np.uint8)
        info = np.zeros((self.n, ABI.INFO_DIM), np.float32)
        self._chk(self.lib.avr_step(self.h, act.ctypes.data, obs.ctypes.data, rew.ctypes.data, done.ctypes.data, info.ctypes.data))
        return obs, rew, done.astype(bool), info

    # device-pointer variants (torch tensors' data_ptr()); asynchronous on the handle's stream
    def step_device(self, d_act, d_obs, d_rew, d_done, d_info):
        self._chk(self.lib.avr_step_device(self.h, d_act, d_obs, d_rew, d_done, d_info))

    def step_random_device(self, t, d_obs=None, d_rew=None, d_done=None, d_info=None):
        self._chk(self.lib.avr_step_random_device(self.h, int(t), d_obs, d_rew, d_done, d_info))

    def rollout_random_device(self, t0, n, d_obs=None, d_rew=None, d_done=None, d_info=None, stacked=False):
        """n device-random steps from step index t0 (= n step_random_device calls, bit for bit); the
        env groups are joined at the end only.  stacked: step k's outputs to slot k of [n, E, ...]
        device arrays (all four required)."""
        self._chk(self.lib.avr_rollout_random_device(self.h, int(t0), int(n), d_obs, d_rew, d_done, d_info, int(bool(stacked))))

    def random_actions_device(self, t, d_act):
        self._chk(self.lib.avr_random_actions_device(self.h, int(t), d_act))

    # ---- the policy on the device (include/avr.h avr_policy_*)
    def policy_set(self, desc):
        """Install a policy: desc is policy_eval.policy_desc's dict (obs_dim, act_dim, hidden,
        n_layers, clip_obs, eps and the float32 arrays of avr_policy_desc.ARRAYS, None = absent).
        Later calls overwrite the weights in stream order; no graph is re-captured."""
        d = avr_policy_desc(obs_dim=int(desc['obs_dim']), act_dim=int(desc['act_dim']), hidden=int(desc['hidden']),
                            n_layers=int(desc.get('n_layers', 2)), clip_obs=float(desc.get('clip_obs', 10.0)), eps=float(desc.get('eps', 1e-8)))
        keep = []
        for k in avr_policy_desc.ARRAYS:
            a = desc.get(k)
            if a is not None:
                a = np.ascontiguousarray(a, np.float32)
                keep.append(a)
                setattr(d, k, a.ctypes.data)
        self._chk(self.lib.avr_policy_set(self.h, C.byref(d)))

    def policy_act_device(self, t, d_obs, deterministic, d_act, d_logp=None, d_value=None):
        """One forward over all envs at step index t (device pointers; d_act None: the value alone)."""
        self._chk(self.lib.avr_policy_act_device(self.h, int(t), d_obs, int(bool(deterministic)), d_act, d_logp, d_value))

    def rollout_policy_device(self, t0, n, d_obs0, deterministic, d_obs, d_act, d_logp, d_value, d_rew, d_done, d_info):
        """n steps from step index t0 with the installed policy in the loop (= n x {policy_act_device;
        step_device}, bit for bit): d_obs0 (None: the handle's observation buffer) is what step t0's
        policy sees; d_obs [n+1, E, obs], d_value [n+1, E] (or None), d_act / d_logp (or None) / d_rew /
        d_done / d_info [n, E, ...] are stacked device arrays."""
        self._chk(self.lib.avr_rollout_policy_device(self.h, int(t0), int(n), d_obs0, int(bool(deterministic)), d_obs, d_act, d_logp, d_value,
                                                     d_rew, d_done, d_info))

    # ---- device-side episode rollover from a reset-state pool (include/avr.h avr_rollover_*)
    def reset_pool_set(self, S, obs):
        """Install (or, with at most as many rows as the first pool, replace) the reset-state pool:
        S (n_pool, state words) settled reset states as get_state returns them, obs (n_pool, obs_dim)
        their reset observations.  No graph is re-captured."""
        S = np.ascontiguousarray(S, np.float32)
        obs = np.ascontiguousarray(obs, np.float32)
        assert S.ndim == 2 and S.shape[1] == self.words and obs.shape == (len(S), self.obs_dim)
        self._chk(self.lib.avr_reset_pool_set(self.h, int(len(S)), S.ctypes.data, obs.ctypes.data))

    def rollover_enable(self, on=True):
        """The rollover mode of the rollouts: envs a step finishes take their next state from the pool."""
        self._chk(self.lib.avr_rollover_enable(self.h, int(bool(on))))

    def rollover_device(self, d_done, d_obs):
        """Roll over the envs with d_done[e] != 0 and rewrite their d_obs rows (device pointers; asynchronous)."""
        self._chk(self.lib.avr_rollover_device(self.h, d_done, d_obs))

    def rollover_buffers(self):
        """Device pointers (term_obs [n_envs, obs_dim] float32, term_value [n_envs] float32, episode
        [n_envs] int32) of the handle's rollover rows."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self.lib.avr_rollover_buffers(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def rollover_set_episodes(self, episodes):
        ep = np.ascontiguousarray(episodes, np.int32).reshape(self.n)
        self._chk(self.lib.avr_rollover_set_episodes(self.h, ep.ctypes.data))

    # ---- the PPO update on the device (include/avr.h avr_gae_device, avr_ppo_*)
    def gae_device(self, n, gamma, lam, bootstrap, d_rew, d_done, d_value, d_adv, d_ret):
        """Advantages and returns of a rollout's stacked [n, n_envs] device arrays (d_value [n+1, n_envs]);
        bootstrap: a done bootstraps from the handle's terminal-value row instead of cutting the return."""
        self._chk(self.lib.avr_gae_device(self.h, int(n), float(gamma), float(lam), int(bool(bootstrap)), d_rew, d_done, d_value, d_adv, d_ret))

    def ppo_reset(self):
        """Allocate / zero the optimiser state (Adam's moments, step count, gradient, statistics)."""
        self._chk(self.lib.avr_ppo_reset(self.h))

    @staticmethod
    def ppo_batch(n, E, **ptrs):
        """avr_ppo_batch of device pointers obs, act, logp, value, adv, ret (None: absent)."""
        b = avr_ppo_batch(n=int(n), E=int(E))
        for k in avr_ppo_batch.ARRAYS:
            setattr(b, k, ptrs.get(k))
        return b

    @staticmethod
    def ppo_params(p):
        """avr_ppo_params from a dict with its field names (avr/ppo.py DEFAULTS has them all)."""
        q = avr_ppo_params(norm_adv=int(bool(p['norm_adv'])), clip_value=int(bool(p['clip_value'])))
        for k in avr_ppo_params.FLOATS:
            setattr(q, k, float(p[k]))
        return q

    def ppo_grad_device(self, batch, params, minibatch, n_minibatch, d_perm=None):
        """Gradient of one minibatch into the handle's gradient block (batch: ppo_batch, params: ppo_params)."""
        self._chk(self.lib.avr_ppo_grad_device(self.h, C.byref(batch), C.byref(params), int(minibatch), int(n_minibatch), d_perm))

    def ppo_adam_device(self, params):
        """Clip the gradient block's norm and take one Adam step on the weight block in place."""
        self._chk(self.lib.avr_ppo_adam_device(self.h, C.byref(params)))

    def ppo_update_device(self, batch, params, epochs, n_minibatch, d_perm=None):
        """epochs x n_minibatch {gradient; Adam} with no host synchronisation (d_perm: int32 [epochs, N])."""
        self._chk(self.lib.avr_ppo_update_device(self.h, C.byref(batch), C.byref(params), int(epochs), int(n_minibatch), d_perm))

    def ppo_advstat_device(self, batch):
        """The batch's advantage mean / std into the handle's cache (what minibatch 0 of ppo_grad_device computes)."""
        self._chk(self.lib.avr_ppo_advstat_device(self.h, C.byref(batch)))

    def ppo_grad_segment_device(self, batch, params, minibatch, n_minibatch, d_perm, segment, d_seg):
        """Segment `segment` (of PPO_SEGMENTS) of a minibatch: its share of the gradient and of the statistics
        into the device row d_seg [PPO_SEG_WORDS]; the handle's gradient block is not touched."""
        self._chk(self.lib.avr_ppo_grad_segment_device(self.h, C.byref(batch), C.byref(params), int(minibatch), int(n_minibatch), d_perm, int(segment), d_seg))

    def ppo_combine_device(self, params, d_segs):
        """The handle's gradient block and next statistics row from the device rows d_segs [PPO_SEGMENTS,
        PPO_SEG_WORDS], added in ascending segment order in double; ppo_adam_device follows."""
        self._chk(self.lib.avr_ppo_combine_device(self.h, C.byref(params), d_segs))

    def ppo_buffers(self):
        """Device pointers (grad, m, v: ppo_words() float32 each; stats [PPO_STATS_ROWS, PPO_STAT_WORDS])."""
        p = [C.c_void_p() for _ in range(4)]
        self._chk(self.lib.avr_ppo_buffers(self.h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def ppo_words(self):
        return int(self.lib.avr_ppo_words())

    def policy_block(self):
        """Device pointer of the weight block (ppo_words() float32; None before policy_set)."""
        return self.lib.avr_policy_block(self.h)

    def policy_get(self):
        """The installed policy's weights read back from the device: policy_set's dict (float32 arrays in
        torch.nn.Linear's orientation; the critic's / ob_rms's entries None when absent)."""
        o = avr_policy_out()
        self._chk(self.lib.avr_policy_get(self.h, C.byref(o)))         # (all pointers NULL: the dimensions)
        h, od, ad = int(o.hidden), self.obs_dim, self.act_dim
        shapes = dict(ob_mean=(od,), ob_var=(od,), a_w1=(h, od), a_b1=(h,), a_w2=(h, h), a_b2=(h,), mu_w=(ad, h), mu_b=(ad,), logstd=(ad,),
                      c_w1=(h, od), c_b1=(h,), c_w2=(h, h), c_b2=(h,), c_w3=(1, h), c_b3=(1,))
        d = dict(obs_dim=od, act_dim=ad, hidden=h, n_layers=2, clip_obs=float(o.clip_obs), eps=float(o.eps))
        for k in avr_policy_out.ARRAYS:
            absent = (k.startswith('c_') and not o.has_critic) or (k.startswith('ob_') and not o.has_ob_rms)
            d[k] = None if absent else np.zeros(shapes[k], np.float32)
            if d[k] is not None:
                setattr(o, k, d[k].ctypes.data)
        self._chk(self.lib.avr_policy_get(self.h, C.byref(o)))
        return d

    def policy_obs_norm_device(self, d_mean, d_var):
        """Rewrite the weight block's ob_rms rows from device float32 arrays [obs_dim] in stream order."""
        self._chk(self.lib.avr_policy_obs_norm_device(self.h, d_mean, d_var))

    # ---- reward normalisation and episode statistics (include/avr.h avr_reward_norm_device, avr_episode_stats_device)
    def reward_norm_device(self, n, gamma, clip_rew, eps, update, d_rew, d_done, d_rew_out):
        """VecNormalize's reward path over a rollout's stacked [n, n_envs] device arrays: d_rew_out (may be
        d_rew) = clamp(rew / sqrt(var + eps), +-clip_rew) with the running variance of the discounted return;
        update False: eval mode, the carried return and statistics stay untouched."""
        self._chk(self.lib.avr_reward_norm_device(self.h, int(n), float(gamma), float(clip_rew), float(eps), int(bool(update)), d_rew, d_done, d_rew_out))

    def episode_stats_device(self, n, d_rew, d_done, d_info, d_row=None):
        """Advance the per-env episode accumulators over a rollout's stacked device arrays; d_row (device
        float64 [EPSTAT_WORDS], columns EPISODE_STATS; None: only the handle's own row) receives the
        aggregate over the episodes closed in this call."""
        self._chk(self.lib.avr_episode_stats_device(self.h, int(n), d_rew, d_done, d_info, d_row))

    def train_stats_reset(self):
        """Allocate / zero the carried rows of the two calls above; the return's moments become (0, 1, 1e-4)."""
        self._chk(self.lib.avr_train_stats_reset(self.h))

    def train_stats_buffers(self):
        """Device pointers (R [n_envs] float64, (mean, var, count) [3] float64, the per-env episode rows
        [len(EPISODE_ENV_ROWS), n_envs] of 4-byte words, the last aggregate row [EPSTAT_WORDS] float64)."""
        p = [C.c_void_p() for _ in range(4)]
        self._chk(self.lib.avr_train_stats_buffers(self.h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    # ---- human height variants (include/avr.h avr_human_variants_set)
    def human_variants_set(self, records):
        """Install the handle's height variants: records is a list of model_compiler.
        human_variant_records dicts (at most MAX_HUMAN_VARIANTS; empty: the base handle again).  A
        state row selects variant v with the value 2 + v in its T_GENDER word (0 / 1: the handle's
        base male / female).  Call it before the first state upload."""
        n = len(records)
        arr = (avr_human_variant * max(n, 1))()
        keep = []
        for i, R in enumerate(records):
            v = arr[i]
            v.gender, v.height = int(R['gender']), float(R['height'])
            v.n_gshapes, v.n_hbodies = len(R['shapes']), len(R['bodies'])
            for k in avr_human_variant.ARRAYS:
                a = R.get(k)
                if a is not None and np.size(a):
                    a = np.ascontiguousarray(a, np.float32)
                    keep.append(a)
                    setattr(v, k, a.ctypes.data)
        self._chk(self.lib.avr_human_variants_set(self.h, n, C.cast(arr, C.c_void_p) if n else None))

    def human_variants(self):
        """[(gender 0 / 1, height)] of the loaded variants, as the library holds them."""
        out = []
        for v in range(int(self.lib.avr_human_variants(self.h))):
            g, h = C.c_int32(), C.c_float()
            self._chk(self.lib.avr_human_variant_info(self.h, v, C.byref(g), C.byref(h)))
            out.append((int(g.value), float(h.value)))
        return out

    def sync(self):
        self._chk(self.lib.avr_sync(self.h))

    def stream(self):
        return self.lib.avr_stream(self.h)

    def env_groups(self):
        return int(self.lib.avr_env_groups(self.h))

    def dyn_split(self):
        """1 when the sub-steps run the dynamics role in the pair launch (AVR_DYN_SPLIT, per-task default)."""
        return int(self.lib.avr_dyn_split(self.h))

    def pairs_flat(self):
        """1 when the pair kernel enumerates the child shape pairs in flat passes (AVR_PAIRS_FLAT, per-task default)."""
        return int(self.lib.avr_pairs_flat(self.h))

    def np_hot(self):
        """1 when the narrowphase starts the contact pool's sphere-hull pairs first (AVR_NP_HOT, per-task default)."""
        return int(self.lib.avr_np_hot(self.h))

    def coop_wsup(self):
        """1 when the cooperative narrowphase takes hull supports wave-wide (AVR_COOP_WSUP, per-task default)."""
        return int(self.lib.avr_coop_wsup(self.h))

    def graph_captures(self):
        """HIP-graph captures this handle has made (one per distinct output-buffer key)."""
        return int(self.lib.avr_graph_captures(self.h))

    def profile_kernels(self, enable=True):
        self._chk(self.lib.avr_profile_kernels(self.h, int(bool(enable))))

    def kernel_times(self):
        """{kernel: (total_ms, launches)} accumulated since profile_kernels(True)."""
        ms = np.zeros(8, np.float64)
        n = np.zeros(8, np.int64)
        self._chk(self.lib.avr_kernel_times(self.h, ms.ctypes.data, n.ctypes.data))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(self.kernel_kinds) if n[i]}

    # ---- state queries (include/avr.h avr_get_*)
    def n_dof(self):
        return int(self.lib.avr_n_dof(self.h))

    def get_q(self):
        """(q, qd), each (n_envs, n_dof): robot DoFs, then the articulated human chain's."""
        nd = self.n_dof()
        q = np.zeros((self.n, nd), np.float32)
        qd = np.zeros((self.n, nd), np.float32)
        self._chk(self.lib.avr_get_q(self.h, q.ctypes.data, qd.ctypes.data))
        return q, qd

    def get_link_pose(self, link):
        """(n_envs, 7) world COM frame of articulated link `link` (-1: robot base)."""
        out = np.zeros((self.n, 7), np.float32)
        self._chk(self.lib.avr_get_link_pose(self.h, int(link), out.ctypes.data))
        return out

    def get_contact_summary(self):
        """(n_envs, 4): contact points, sum of normal force, robot-human, tool-human."""
        out = np.zeros((self.n, 4), np.float32)
        self._chk(self.lib.avr_get_contact_summary(self.h, out.ctypes.data))
        return out

    def get_flags(self):
        """(n_envs,) int32 health flags (0 = healthy; bits in include/avr.h avr_get_flags)."""
        out = np.zeros(self.n, np.int32)
        self._chk(self.lib.avr_get_flags(self.h, out.ctypes.data))
        return out

    # ---- views (include/avr.h avr_render_device)
    def n_bodies(self):
        return int(self.lib.avr_n_bodies(self.h))

    def body_poses(self):
        """(n_envs, n_bodies, 7) world COM frame of every collision body at the current state: what the
        renderer places the shapes at (p.getBasePositionAndOrientation / p.getLinkState for all bodies)."""
        out = np.zeros((self.n, self.n_bodies(), 7), np.float32)
        self._chk(self.lib.avr_get_body_poses(self.h, out.ctypes.data))
        return out

    def render_set_planes(self, planes4, shape_range2):
        """Install the hulls' face planes: planes4 (n_planes, 4) rows (n, w) of n . x <= w in the shape's
        frame, shape_range2 (n_shapes, 2) rows (first plane, count) (avr/render.py hull_planes)."""
        p = np.ascontiguousarray(planes4, np.float32).reshape(-1, 4)
        r = np.ascontiguousarray(shape_range2, np.int32).reshape(-1, 2)
        self._chk(self.lib.avr_render_set_planes(self.h, int(len(p)), p.ctypes.data if len(p) else None, r.ctypes.data))

    @staticmethod
    def camera_struct(cam):
        """avr_camera from an object with its fields (avr/render.py Camera) or from an avr_camera."""
        if cam is None or isinstance(cam, avr_camera):
            return cam
        c = avr_camera(fov_y_deg=float(cam.fov_y_deg), near=float(cam.near), far=float(cam.far), width=int(cam.width), height=int(cam.height),
                       body=int(cam.body))
        for i in range(3):
            c.eye[i], c.target[i], c.up[i] = float(cam.eye[i]), float(cam.target[i]), float(cam.up[i])
        return c

    def render_device(self, cam, env_ids, depth_ptr, id_ptr, rgb_ptr, n=None):
        """Queue a render of envs env_ids (None: 0 .. n-1, n defaulting to all) through cam into the device
        buffers depth [n, H, W] float32, id [n, H, W] int32, rgb [n, H, W, 3] uint8 (any may be None, not
        all); asynchronous on the handle's stream."""
        c = self.camera_struct(cam)
        ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32).reshape(-1)
        n = (self.n if n is None else int(n)) if ids is None else len(ids)
        self._chk(self.lib.avr_render_device(self.h, None if c is None else C.byref(c), n, None if ids is None else ids.ctypes.data,
                                             depth_ptr, id_ptr, rgb_ptr))

    def render_tile_stats(self, cam, env_ids=None):
        """(n, tiles_y, tiles_x, 2) int32: per 8 x 8 tile the shapes its culled list holds and the hull
        planes one of its pixels tests (include/avr.h avr_render_tile_stats)."""
        c = self.camera_struct(cam)
        ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32).reshape(-1)
        n = self.n if ids is None else len(ids)
        ty, tx = -(-int(c.height) // RENDER_TILE), -(-int(c.width) // RENDER_TILE)
        out = np.zeros((n, ty, tx, 2), np.int32)
        self._chk(self.lib.avr_render_tile_stats(self.h, C.byref(c), n, None if ids is None else ids.ctypes.data, out.ctypes.data))
        return out

    def render_kernel_info(self):
        """{kernel: dict(vgprs, lds_bytes, scratch_bytes)} of the two render kernels."""
        out = np.zeros(8, np.int32)
        self._chk(self.lib.avr_render_kernel_info(self.h, out.ctypes.data))
        return {n: dict(vgprs=int(out[4 * i]), lds_bytes=int(out[4 * i + 2]), scratch_bytes=int(out[4 * i + 3])) for i, n in enumerate(('frames', 'trace'))}

    def kernel_info(self):
        """{kernel: dict(vgprs, lds_bytes, scratch_bytes)} of the step's kernels (include/avr.h)."""
        out = np.zeros(20, np.int32)
        self._chk(self.lib.avr_kernel_info(self.h, out.ctypes.data))
        names = ('pairs', 'narrowphase', 'a', 'b', 'task')
        return {n: dict(vgprs=int(out[4 * i]), lds_bytes=int(out[4 * i + 2]), scratch_bytes=int(out[4 * i + 3])) for i, n in enumerate(names)}


# ---------------------------------------------------------------- Philox4x32-10 (host mirror)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(c, k0, k1):
    """Vectorised Philox4x32-10 on uint64 arrays holding 32-bit values; c: (4, N)."""
    c = [np.asarray(x, np.uint64) & 0xFFFFFFFF for x in c]
    k0 = np.uint64(k0 & 0xFFFFFFFF)
    k1 = np.uint64(k1 & 0xFFFFFFFF)
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        h0, l0 = p0 >> np.uint64(32), p0 & mask
        h1, l1 = p1 >> np.uint64(32), p1 & mask
        c = [h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0]
        k0 = (k0 + np.uint64(W0)) & mask
        k1 = (k1 + np.uint64(W1)) & mask
    return c


def random_actions(seed, env_ids, t, act_dim=ABI.ACT_DIM):
    """a[e, j] ~ U(-1,1) float32 from Philox4x32-10 keyed by (seed, env, t) -- identical to the
    device generator (examples/random_actions.py semantics with a counter-based stream)."""
    env_ids = np.asarray(env_ids, np.uint64)
    out = np.zeros((len(env_ids), act_dim), np.float32)
    for blk in range((act_dim + 3) // 4):
        c = [env_ids, np.full_like(env_ids, t & 0xFFFFFFFF), np.full_like(env_ids, blk), np.full_like(env_ids, (t >> 32) & 0xFFFFFFFF)]
        r = philox4x32_10(c, seed, seed >> 32)
        for k in range(4):
            j = 4 * blk + k
            if j < act_dim:
                x = (r[k] >> np.uint64(8)).astype(np.float32)
                out[:, j] = x * np.float32(1.0 / 16777216.0) * np.float32(2.0) - np.float32(1.0)
    return out


def policy_noise(seed, env_ids, t, act_dim=ABI.ACT_DIM):
    """eps[e, j] ~ N(0, 1), float64: the host mirror of the device policy's sampling noise
    (csrc/avr_policy.hip philox_normal).  Philox4x32-10 keyed by (seed, env, t) as random_actions,
    with the top bit of counter word 2 set (random_actions' word 2 is j >> 2: never set), so the
    two streams share no counter.  Block j >> 2 gives four words; words (0, 1) make the Box-Muller
    pair of j & 3 = 0 (cos) and 1 (sin), words (2, 3) that of j & 3 = 2 and 3, with
    u1 = ((x >> 8) + 0.5) / 2^24 formed in float32 as on the device (never 0) and
    u2 = (x' >> 8) / 2^24; the logarithm, root and cos / sin are float64 here."""
    env_ids = np.asarray(env_ids, np.uint64)
    out = np.zeros((len(env_ids), act_dim), np.float64)
    for blk in range((act_dim + 3) // 4):
        c = [env_ids, np.full_like(env_ids, t & 0xFFFFFFFF), np.full_like(env_ids, 0x80000000 | blk), np.full_like(env_ids, (t >> 32) & 0xFFFFFFFF)]
        r = philox4x32_10(c, seed, seed >> 32)
        for pair in range(2):
            xa, xb = r[2 * pair] >> np.uint64(8), r[2 * pair + 1] >> np.uint64(8)
            u1 = ((xa.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)).astype(np.float64)
            u2 = xb.astype(np.float64) / 16777216.0
            rad, th = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
            for k, z in ((0, rad * np.cos(th)), (1, rad * np.sin(th))):
                j = 4 * blk + 2 * pair + k
                if j < act_dim:
                    out[:, j] = z
    return out


def rollover_index(seed, env_ids, episodes, n_pool):
    """Pool row an env's rollover takes, int64 (len(env_ids),): the host mirror of the device rollover's
    pick (csrc/avr_rollover.hip rollover_env).  Word 0 of Philox4x32-10 keyed by seed on the counter
    {env, episode lo, 0x40000000, episode hi}, modulo n_pool; env_ids are global ids (env_offset + e),
    episodes the counters before the increment (a scalar or one per env).  random_actions' counter
    word 2 is 0 or 1 and policy_noise's has the top bit set, so the three streams share no counter."""
    if int(n_pool) < 1:
        raise ValueError('rollover_index: n_pool must be >= 1')
    env_ids = np.asarray(env_ids, np.uint64)
    ep = np.broadcast_to(np.asarray(episodes, np.int64), env_ids.shape).astype(np.uint64)
    c = [env_ids, ep & np.uint64(0xFFFFFFFF), np.full_like(env_ids, 0x40000000), ep >> np.uint64(32)]
    r = philox4x32_10(c, seed, seed >> 32)
    return (r[0] % np.uint64(n_pool)).astype(np.int64)


def hull_support_table(verts, G=16):
    """Host support table of one hull (avr_hull_support_table): (cell[6G^2, 2], idx[total])."""
    lib = load()
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    cell = np.zeros((6 * G * G, 2), dtype=np.int32)
    tot = lib.avr_hull_support_table(v.ctypes.data, len(v), G, cell.ctypes.data, None, 0)
    if tot < 0:
        raise RuntimeError('avr_hull_support_table failed')
    idx = np.zeros(max(tot, 1), dtype=np.int32)
    lib.avr_hull_support_table(v.ctypes.data, len(v), G, cell.ctypes.data, idx.ctypes.data, tot)
    return cell, idx[:tot]
