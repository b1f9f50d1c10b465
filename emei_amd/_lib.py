"""ctypes binding of libemei_hip.so (C ABI: include/emei_hip.h).

The HIP library is the product path: there is no CPU or PyTorch fallback.  If the shared object is
missing or does not export the ABI, importing this module's `lib()` raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# EMEI_HIP_LIB lets a developer A/B two builds of the same ABI inside one process launch; the default
# is the in-tree library next to this file.
LIB_PATH = os.environ.get("EMEI_HIP_LIB") or os.path.join(_HERE, "libemei_hip.so")

# enum emei_env_id
ENV_IDS = {
    "CartPoleSwingUp": 0,
    "CartPoleBalancing": 1,
    "ReboundInvertedPendulumBalancing": 2,
    "BoundaryInvertedPendulumBalancing": 3,
    "ReboundInvertedPendulumSwingUp": 4,
    "BoundaryInvertedPendulumSwingUp": 5,
    "HalfCheetahRunning": 6,
    "ReboundInvertedDoublePendulumBalancing": 7,
    "BoundaryInvertedDoublePendulumBalancing": 8,
    "ReboundInvertedDoublePendulumSwingUp": 9,
    "BoundaryInvertedDoublePendulumSwingUp": 10,
    "HopperRunning": 11,
}
PRECISION_REF, PRECISION_F32 = 0, 1
ACT_U8, ACT_I32, ACT_I64, ACT_F32 = 0, 1, 2, 3
FLAG_AUTO_RESET = 1
DONE_TERMINAL, DONE_TRUNCATED = 1, 2
OK, ERR_INVALID, ERR_HIP, ERR_UNSUPPORTED, ERR_STATE = 0, -1, -2, -3, -4
ABI_VERSION = 8
IO_F32, IO_F64 = 0, 1  # enum emei_io_dtype
REWARD_BATCH_CTRL_COST = 1  # flag of emei_reward_io (half_cheetah.py:61 / hopper.py:98: np.sum over the whole batch)
# enum emei_kernel_id (emei_last_rollout_kernel)
KERNEL_NAMES = {0: "none", 1: "pend_rollout_staged_kernel<freq1>", 2: "pend_rollout_staged_kernel", 3: "pend_rollout_kernel<full>",
                4: "pend_rollout_kernel", 5: "body_rollout_kernel", 6: "body_rollout_kernel<rk4>",
                7: "body_rollout_kernel (chunked work items)", 8: "body_rollout_kernel<rk4> (chunked work items)",
                9: "pend_rollout_staged_peers_kernel<freq1>", 10: "pend_rollout_staged_peers_kernel", 11: "pend_mpc_mppi_kernel",
                12: "pend_mpc_cem_kernel", 13: "body_mpc_mppi_kernel", 14: "body_mpc_cem_kernel"}
# ... and the ids of emei_rollout_policy's kernels, a table of their own (KERNEL_NAMES stays the 15 ids of emei_rollout and the fused
# controllers); kernel_name() looks an id up in both
POLICY_KERNEL_NAMES = {15: "pend_policy_rollout_kernel", 16: "body_policy_rollout_kernel", 17: "body_policy_rollout_kernel<rk4>"}
# ... and those of emei_rollout_policy_noisy, likewise a table of their own
POLICY_NOISY_KERNEL_NAMES = {18: "pend_policy_rollout_noisy_kernel", 19: "body_policy_rollout_noisy_kernel",
                             20: "body_policy_rollout_noisy_kernel<rk4>"}
# ... and those of emei_rollout_policy_deep (one kernel per family, with or without noise), likewise
POLICY_DEEP_KERNEL_NAMES = {21: "pend_policy_rollout_deep_kernel", 22: "body_policy_rollout_deep_kernel",
                            23: "body_policy_rollout_deep_kernel<rk4>"}
# ... and those of emei_mpc_policy (enum emei_kernel_id_mpc_policy), likewise
MPC_POLICY_KERNEL_NAMES = {24: "pend_mpc_policy_kernel", 25: "body_mpc_policy_kernel"}


def kernel_name(kernel_id):
    """name of an enum emei_kernel_id value (emei_last_rollout_kernel)"""
    for table in (KERNEL_NAMES, POLICY_KERNEL_NAMES, POLICY_NOISY_KERNEL_NAMES, POLICY_DEEP_KERNEL_NAMES, MPC_POLICY_KERNEL_NAMES):
        if kernel_id in table:
            return table[kernel_id]
    raise KeyError(kernel_id)


KERNEL_PEND_STAGED_FREQ1, KERNEL_PEND_STAGED, KERNEL_PEND_GENERIC_FULL, KERNEL_PEND_GENERIC, KERNEL_BODY, KERNEL_BODY_RK4 = 1, 2, 3, 4, 5, 6
KERNEL_BODY_CHUNKED, KERNEL_BODY_RK4_CHUNKED = 7, 8
KERNEL_PEND_STAGED_PEERS_FREQ1, KERNEL_PEND_STAGED_PEERS = 9, 10
KERNEL_PEND_MPC_MPPI = 11
KERNEL_PEND_MPC_CEM = 12
KERNEL_BODY_MPC_MPPI, KERNEL_BODY_MPC_CEM = 13, 14  # the InvertedDoublePendulum's fused controllers
KERNEL_PEND_POLICY, KERNEL_BODY_POLICY, KERNEL_BODY_POLICY_RK4 = 15, 16, 17  # emei_rollout_policy
POLICY_OUT_CLIP, POLICY_OUT_TANH = 0, 1  # enum emei_policy_out
KERNEL_PEND_POLICY_NOISY, KERNEL_BODY_POLICY_NOISY, KERNEL_BODY_POLICY_NOISY_RK4 = 18, 19, 20  # emei_rollout_policy_noisy
POLICY_NOISE_GAUSS, POLICY_NOISE_GAUSS_HEAD, POLICY_NOISE_EPS_GREEDY = 0, 1, 2  # enum emei_policy_noise_mode
POLICY_MAX_HIDDEN = 1024  # EMEI_POLICY_MAX_HIDDEN
KERNEL_PEND_POLICY_DEEP, KERNEL_BODY_POLICY_DEEP, KERNEL_BODY_POLICY_DEEP_RK4 = 21, 22, 23  # emei_rollout_policy_deep
POLICY_DEEP_MAX_HIDDEN = 256  # EMEI_POLICY_DEEP_MAX_HIDDEN
KERNEL_PEND_MPC_POLICY, KERNEL_BODY_MPC_POLICY = 24, 25  # enum emei_kernel_id_mpc_policy (emei_mpc_policy)
MPC_POLICY_ACT_BEST, MPC_POLICY_ACT_MEAN = 0, 1  # enum emei_mpc_policy_act
MPC_MAX_HORIZON = 256  # EMEI_MPC_MAX_HORIZON
MAX_OBS_PEERS = 8  # EMEI_MAX_OBS_PEERS
# enum emei_ode_method: `method` of ODE_approximation (base_control.py:133-173), classic control only
ODE_METHODS = {"euler": 0, "rk4": 1}
NEXT_OBS_ODE_RK4 = 0x100  # flag on emei_next_obs_io's `integrator`
# enum emei_integrator (mujoco_env.py:70-79) / enum emei_noise_layout
INTEGRATORS = {"euler": 0, "semi_implicit_euler": 1, "rk4": 2}
NOISE_IID, NOISE_SHARED = 0, 1
# enum emei_solver
SOLVERS = {"newton": 0, "sweep1": 1}
CONFIG_SIZE_V1 = 64
MAX_STATE_DIM = 32
MAX_ENV_PARAMS = 8
# enum emei_env_param
ENV_PARAMS = {"forward_reward_weight": 0, "ctrl_cost_weight": 1, "healthy_reward": 2, "terminate_when_unhealthy": 3,
              "healthy_state_lo": 4, "healthy_state_hi": 5, "healthy_z_lo": 6, "healthy_z_hi": 7}


class EmeiConfig(C.Structure):
    """struct emei_config (include/emei_hip.h)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("env_id", C.c_int32),
        ("n_envs", C.c_int64),
        ("freq_rate", C.c_int32),
        ("precision", C.c_int32),
        ("real_time_scale", C.c_double),
        ("max_episode_steps", C.c_int32),
        ("device", C.c_int32),
        ("seed", C.c_uint64),
        ("env_index_offset", C.c_uint64),
        ("init_noise", C.c_double),
        # ABI version 2
        ("integrator", C.c_int32),
        ("noise_layout", C.c_int32),
        ("init_sigma", C.c_float * MAX_STATE_DIM),
        ("obs_sigma", C.c_float * MAX_STATE_DIM),
        # struct_size 400: constructor parameters of the reward / terminal functions
        ("env_param_mask", C.c_uint32),
        ("solver", C.c_uint32),
        ("env_params", C.c_double * MAX_ENV_PARAMS),
        # struct_size 408 (ABI 6)
        ("ode_method", C.c_int32),
        ("rollout_chunk_steps", C.c_int32),
    ]


class EmeiPolicy(C.Structure):
    """struct emei_policy (include/emei_hip.h): the weights are device pointers."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("hidden", C.c_int32),
        ("out_mode", C.c_int32),
        ("reserved", C.c_int32),
        ("w1", C.c_void_p),
        ("b1", C.c_void_p),
        ("w2", C.c_void_p),
        ("b2", C.c_void_p),
    ]


class EmeiPolicyDeep(C.Structure):
    """struct emei_policy_deep (include/emei_hip.h): two hidden layers; the weights are device pointers."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("hidden1", C.c_int32),
        ("hidden2", C.c_int32),
        ("out_mode", C.c_int32),
        ("w1", C.c_void_p),
        ("b1", C.c_void_p),
        ("w2", C.c_void_p),
        ("b2", C.c_void_p),
        ("w3", C.c_void_p),
        ("b3", C.c_void_p),
        ("reserved", C.c_int64),
    ]


class EmeiPolicyNoise(C.Structure):
    """struct emei_policy_noise (include/emei_hip.h): std / ws / bs are device pointers."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mode", C.c_int32),
        ("seed", C.c_uint64),
        ("sigma", C.c_double),
        ("std", C.c_void_p),
        ("ws", C.c_void_p),
        ("bs", C.c_void_p),
        ("log_std_min", C.c_float),
        ("log_std_max", C.c_float),
        ("reserved", C.c_int32),
    ]


# name -> (restype, argtypes); every symbol include/emei_hip.h declares
_vp, _i32, _i64, _u32, _u64, _dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double
SYMBOLS = {
    "emei_create": (C.c_int, [C.POINTER(EmeiConfig), C.POINTER(_vp)]),
    "emei_destroy": (C.c_int, [_vp]),
    "emei_last_error": (C.c_char_p, []),
    "emei_abi_version": (C.c_int, []),
    "emei_model_constants": (C.c_int, [C.c_int, _vp, C.c_int]),
    "emei_model_invweights": (C.c_int, [C.c_int, _vp, C.c_int]),
    "emei_env_dims": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "emei_reset": (C.c_int, [_vp, _u64, _vp]),
    "emei_set_seed": (C.c_int, [_vp, _u64]),
    "emei_get_solver_cap_hits": (C.c_int, [_vp, _vp, _vp]),
    "emei_get_rollout_faults": (C.c_int, [_vp, _vp, _vp]),
    "emei_last_rollout_kernel": (C.c_int, [_vp]),
    "emei_set_obs_peers": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _i64, _i64, _i32]),
    "emei_peer_buffer_create": (C.c_int, [C.c_int, _u64, C.POINTER(_vp), _vp]),
    "emei_peer_buffer_open": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "emei_peer_buffer_close": (C.c_int, [C.c_int, _vp]),
    "emei_peer_buffer_destroy": (C.c_int, [C.c_int, _vp]),
    "emei_set_state": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "emei_get_state": (C.c_int, [_vp, _vp, _vp]),
    "emei_get_obs": (C.c_int, [_vp, _vp, _vp]),
    "emei_freeze": (C.c_int, [_vp, _vp]),
    "emei_unfreeze": (C.c_int, [_vp, _vp]),
    "emei_step": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, _u32, _vp]),
    "emei_step_host": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _u32, _vp]),
    "emei_rollout": (C.c_int, [_vp, _i32, _vp, C.c_int, _vp, _vp, _vp, _u32, _vp]),
    "emei_evaluate_sequences": (C.c_int, [_vp, _i32, _i32, _vp, C.c_int, _dbl, _vp, _vp, _vp, _vp, _vp]),
    "emei_plan_shooting_workspace_bytes": (_i64, [_i64, _i32]),
    "emei_sample_candidates": (C.c_int, [_vp, _i32, _i32, _u64, _vp, _dbl, _vp, C.c_int, _vp]),
    "emei_plan_shooting": (C.c_int, [_vp, _i32, _i32, _u64, _vp, _dbl, _dbl, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "emei_plan_mppi_workspace_bytes": (_i64, [_i64, _i32]),
    "emei_plan_mppi": (C.c_int, [_vp, _i32, _i32, _u64, _vp, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "emei_sample_candidates_sigma": (C.c_int, [_vp, _i32, _i32, _u64, _vp, _vp, _vp, C.c_int, _vp]),
    "emei_plan_cem_workspace_bytes": (_i64, [_i64, _i32]),
    "emei_plan_cem": (C.c_int, [_vp, _i32, _i32, _i32, _u64, _vp, _dbl, _vp, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "emei_mpc_mppi_workspace_bytes": (_i64, [_i64, _i32]),
    "emei_mpc_mppi": (C.c_int, [_vp, _i32, _i32, _i32, _u64, _vp, _dbl, _dbl, _dbl, C.c_float, C.c_float, C.c_float, _vp, _vp, C.c_int,
                                _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "emei_mpc_cem_workspace_bytes": (_i64, [_i64, _i32]),
    "emei_mpc_cem": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _u64, _vp, _dbl, _dbl, _dbl, C.c_float, C.c_float, C.c_float, _vp, _vp,
                               C.c_int, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "emei_rollout_policy": (C.c_int, [_vp, _i32, C.POINTER(EmeiPolicy), _vp, C.c_int, _vp, _vp, _vp, _u32, _vp]),
    "emei_rollout_policy_noisy": (C.c_int, [_vp, _i32, C.POINTER(EmeiPolicy), C.POINTER(EmeiPolicyNoise), _vp, C.c_int, _vp, _vp, _vp, _u32,
                                            _vp]),
    "emei_evaluate_policies": (C.c_int, [_vp, _i32, _i32, C.POINTER(EmeiPolicy), _dbl, _vp, _vp, _vp, _vp, _vp]),
    "emei_plan_policy_workspace_bytes": (_i64, [_i64, _i32]),
    "emei_plan_policy": (C.c_int, [_vp, _i32, _i32, C.POINTER(EmeiPolicy), C.POINTER(EmeiPolicyNoise), _dbl, _dbl, _vp, _vp, _vp, C.c_int,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "emei_rollout_policy_deep": (C.c_int, [_vp, _i32, C.POINTER(EmeiPolicyDeep), C.POINTER(EmeiPolicyNoise), _vp, C.c_int, _vp, _vp, _vp, _u32,
                                           _vp]),
    "emei_evaluate_policies_deep": (C.c_int, [_vp, _i32, _i32, C.POINTER(EmeiPolicyDeep), _dbl, _vp, _vp, _vp, _vp, _vp]),
    "emei_plan_policy_deep": (C.c_int, [_vp, _i32, _i32, C.POINTER(EmeiPolicyDeep), C.POINTER(EmeiPolicyNoise), C.POINTER(EmeiPolicyDeep),
                                        _dbl, _dbl, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the open-loop plan calls with a terminal value: the plain call's arguments with `value` after `discount`
    "emei_plan_value_workspace_bytes": (_i64, [_i64, _i32]),
    "emei_evaluate_sequences_value": (C.c_int, [_vp, _i32, _i32, _vp, C.c_int, _dbl, C.POINTER(EmeiPolicyDeep), _vp, _vp, _vp, _vp, _vp]),
    "emei_plan_shooting_value": (C.c_int, [_vp, _i32, _i32, _u64, _vp, _dbl, _dbl, C.POINTER(EmeiPolicyDeep), _vp, _vp, _vp, C.c_int, _vp,
                                           _vp, _vp, _vp, _vp]),
    "emei_plan_mppi_value": (C.c_int, [_vp, _i32, _i32, _u64, _vp, _dbl, _dbl, C.POINTER(EmeiPolicyDeep), _dbl, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp]),
    "emei_plan_cem_value": (C.c_int, [_vp, _i32, _i32, _i32, _u64, _vp, _dbl, _vp, _dbl, C.POINTER(EmeiPolicyDeep), _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp]),
    "emei_mpc_policy_workspace_bytes": (_i64, [_i64, _i32]),
    "emei_mpc_policy": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(EmeiPolicy), C.POINTER(EmeiPolicyNoise), _u64, _i32, _dbl, _dbl, _vp, _vp,
                                  C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "emei_compact_done": (C.c_int, [_vp, _vp, _vp, _vp]),
    "emei_get_counters": (C.c_int, [_vp, _vp, _vp, _vp]),
    "emei_episode_init_obs": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "emei_reward": (C.c_int, [C.c_int, _i64, _vp, _vp, _vp, _dbl, _i32, _vp, _vp]),
    "emei_terminal": (C.c_int, [C.c_int, _i64, _vp, _vp, _vp]),
    "emei_reward_ex": (C.c_int, [C.c_int, _i64, _vp, _vp, _vp, _dbl, _i32, _u32, _vp, _vp, _vp]),
    "emei_terminal_ex": (C.c_int, [C.c_int, _i64, _vp, _u32, _vp, _vp, _vp]),
    "emei_next_obs": (C.c_int, [C.c_int, _i64, _vp, _vp, C.c_int, _dbl, _i32, _i32, _vp, _vp]),
    "emei_next_obs_ex": (C.c_int, [C.c_int, _i64, _vp, _vp, C.c_int, _dbl, _i32, _i32, _i32, _vp, _vp]),
    "emei_reward_io": (C.c_int, [C.c_int, _i64, C.c_int, _vp, _vp, _vp, _dbl, _i32, _u32, _vp, _u32, _vp, _vp]),
    "emei_terminal_io": (C.c_int, [C.c_int, _i64, C.c_int, _vp, _u32, _vp, _vp, _vp]),
    "emei_next_obs_io": (C.c_int, [C.c_int, _i64, C.c_int, _vp, _vp, C.c_int, _dbl, _i32, _i32, _i32, _vp, _vp]),
}

_lib = None


class EmeiHipError(RuntimeError):
    pass


def lib():
    """Load libemei_hip.so; fail loudly (no fallback) when it is absent or stale."""
    global _lib
    if _lib is None:
        # torch must be imported first: its bundled HIP runtime and /opt/rocm's share one SONAME, and
        # whichever loads first serves both; loading ours before torch leaves torch without a device.
        import torch  # noqa: F401

        if not os.path.exists(LIB_PATH):
            raise EmeiHipError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C emei_amd/csrc`). emei_amd has no CPU fallback."
            )
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)  # AttributeError if the ABI symbol is not exported
            fn.restype, fn.argtypes = res, args
        if l.emei_abi_version() != ABI_VERSION:
            raise EmeiHipError(f"libemei_hip.so ABI {l.emei_abi_version()} != binding {ABI_VERSION}")
        _lib = l
    return _lib


def pack_env_params(params):
    """{name: value} (names of ENV_PARAMS) -> (mask, c_double[MAX_ENV_PARAMS]); None / {} -> the defaults."""
    arr = (C.c_double * MAX_ENV_PARAMS)()
    mask = 0
    for k, v in (params or {}).items():
        idx = ENV_PARAMS[k]
        arr[idx] = float(v)
        mask |= 1 << idx
    return mask, arr


def check(rc):
    """Map ABI status codes onto the exceptions the reference raises at the same places."""
    if rc == OK:
        return
    msg = lib().emei_last_error().decode()
    if rc == ERR_INVALID:
        raise ValueError(msg)
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == ERR_STATE:
        raise AssertionError(msg)  # `assert self.state is not None`, base_control.py:67
    raise EmeiHipError(msg)
