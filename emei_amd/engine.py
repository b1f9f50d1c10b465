"""Batched env engine: a thin, torch-tensor-facing wrapper of the C ABI handle.

PyTorch is plumbing here (device memory + streams); every computation happens in libemei_hip.so.
"""
import ctypes as C

import torch

from . import _lib as L

_ACT_DTYPES = {torch.uint8: L.ACT_U8, torch.int32: L.ACT_I32, torch.int64: L.ACT_I64, torch.float32: L.ACT_F32}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


# ctrlrange of the continuous envs mpc_mppi serves (inverted_pendulum.xml:23), its default clamp of the nominal
_CTRL_RANGE = {name: (-3.0, 3.0) for name in L.ENV_IDS if name.endswith(("InvertedPendulumBalancing", "InvertedPendulumSwingUp"))}


def _stream():
    """hipStream_t of torch's current stream on the current device (the raw getter avoids building a
    Stream object on every call: 0.3 us instead of 3 us on the per-step path)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _stream_handle(device_index):
    """the same as an integer for a pre-bound ctypes call (emei_step_host)"""
    if _raw_stream is not None:
        return _raw_stream(device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _seed64(seed):
    """a Python int as the ABI's uint64_t seed"""
    return int(seed) & (2**64 - 1)


def env_dims(env_name):
    od, ad, sd = C.c_int(), C.c_int(), C.c_int()
    L.check(L.lib().emei_env_dims(L.ENV_IDS[env_name], C.byref(od), C.byref(ad), C.byref(sd)))
    return od.value, ad.value, sd.value


def _on_device(method):
    """Run an Engine method with the engine's device current (the C ABI refuses a handle used under another
    current device); a plain call when it already is (the per-step path pays one integer compare)."""
    import functools

    @functools.wraps(method)
    def wrapper(self, *a, **k):
        if torch.cuda.current_device() == self.device.index:
            return method(self, *a, **k)
        with torch.cuda.device(self.device):
            return method(self, *a, **k)

    return wrapper


def _sigmas(x, state_dim):
    """float -> the same sigma everywhere; (pos, vel) -> per half; a sequence of state_dim values as given."""
    half = state_dim // 2
    if isinstance(x, (int, float)):
        return [float(x)] * state_dim
    x = [float(v) for v in x]
    if len(x) == 2 and state_dim != 2:
        return [x[0]] * half + [x[1]] * half
    if len(x) != state_dim:
        raise ValueError(f"noise sigmas {x!r}: expected a float, a (pos, vel) pair or {state_dim} values")
    return x


def _plan_policy_checked(engine, H, K, policy, noise, value, discount, temperature, deep):
    """validated (H, K, policy struct, noise struct, value struct or None, discount, temperature or None) of Engine.plan_policy — deep:
    with a policy.DeepMLPPolicy (emei_plan_policy_deep), else with a one-layer policy.MLPPolicy; policy, noise and value are bound
    to `engine` (shapes against the env, the noise mode against the env kind).  Needs no handle."""
    from .policy import DeepMLPPolicy, DeepValueFunction, MLPPolicy, PolicyNoise

    H, K = int(H), int(K)
    if H < 1 or K < 1:
        raise ValueError(f"horizon={H} and n_candidates={K} must be >= 1")
    if deep and not isinstance(policy, DeepMLPPolicy):
        raise TypeError("the two-hidden-layer plan_policy takes an emei_amd.DeepMLPPolicy")
    if not isinstance(policy, MLPPolicy):
        raise TypeError("plan_policy takes an emei_amd.MLPPolicy")
    if not deep and isinstance(policy, DeepMLPPolicy):
        raise ValueError("plan_policy: the two-hidden-layer network (DeepMLPPolicy) is not served by this call yet; "
                         "it takes an MLPPolicy with one hidden layer or none")
    if not isinstance(noise, PolicyNoise):
        raise TypeError("plan_policy takes an emei_amd.PolicyNoise (the exploration noise that makes the candidates differ)")
    if value is not None and not isinstance(value, DeepValueFunction):
        raise TypeError("plan_policy takes an emei_amd.DeepValueFunction as value= (the terminal value network), or None")
    discount = float(discount)
    if not 0.0 < discount <= 1.0:
        raise ValueError(f"discount={discount} is outside (0, 1]")
    if temperature is not None:
        temperature = float(temperature)
        if not (0.0 < temperature < float("inf")):
            raise ValueError(f"temperature={temperature} must be finite and > 0 (None: no weighted mean, no ess)")
    policy.bind(engine)
    # a log-std head reads the last hidden layer (the affine policy: the observation)
    ns = noise.bind(engine).struct(policy.hidden2 if deep else policy.hidden if policy.hidden else policy.obs_dim)
    vs = value.bind(engine).struct() if value is not None else None
    return H, K, policy.struct(), ns, vs, discount, temperature


class Engine:
    """N independent env instances of one kind on one GPU (this rank's shard)."""

    def __init__(self, env_name, n_envs, freq_rate=1, real_time_scale=0.02, precision="ref", max_episode_steps=0,
                 device=None, seed=0, env_index_offset=0, init_noise=0.0, integrator="euler", obs_noise=0.0,
                 noise_layout="iid", env_params=None, solver="newton", ode_method="euler", rollout_chunk_steps=0):
        """init_noise / obs_noise: one sigma, a (qpos sigma, qvel sigma) pair, or one sigma per state coordinate
        (qpos entries then qvel entries): the reduced forms of mujoco_env.py:218-227.
        env_params: {name: value} overriding reward / health constructor defaults (names: _lib.ENV_PARAMS).
        solver: constraint solver of HalfCheetah / Hopper: "newton" (MuJoCo's formulation, converged; the default) or
        "sweep1" (round 1's single Gauss-Seidel sweep).
        ode_method: CartPole only — the `method` of ODE_approximation: "euler" is what the reference's step() always runs
        (base_control.py:73), "rk4" its other branch (:165-170), an explicit opt-in.
        rollout_chunk_steps: rollouts of the one-wave-per-SIMD bodies as (64 envs) x (k steps) work items: 0 = automatic,
        -1 = off, k > 0 = k steps per item (emei_hip.h: emei_config.rollout_chunk_steps); results do not depend on it."""
        if env_name not in L.ENV_IDS:
            raise ValueError(f"unknown env {env_name!r}; known: {sorted(L.ENV_IDS)}")
        if integrator not in L.INTEGRATORS:
            raise NotImplementedError(f"integrator {integrator!r}")  # mujoco_env.py:78-79
        if not torch.cuda.is_available():
            raise L.EmeiHipError("emei_amd needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.env_name, self.n_envs = env_name, int(n_envs)
        self.freq_rate, self.real_time_scale = int(freq_rate), float(real_time_scale)
        self.precision = {"ref": L.PRECISION_REF, "f32": L.PRECISION_F32}[precision]
        self.obs_dim, self.act_dim, self.state_dim = env_dims(env_name)
        self.integrator = integrator
        if solver not in L.SOLVERS:
            raise ValueError(f"solver {solver!r}; known: {sorted(L.SOLVERS)}")
        self.solver = solver
        if ode_method not in L.ODE_METHODS:
            raise NotImplementedError(f"approximation method `{ode_method}` is not suppoerted yet.")  # base_control.py:171-172
        self.ode_method = ode_method
        sig = C.c_float * L.MAX_STATE_DIM
        cfg = L.EmeiConfig(C.sizeof(L.EmeiConfig), L.ENV_IDS[env_name], self.n_envs, self.freq_rate, self.precision,
                           self.real_time_scale, int(max_episode_steps), self.device.index, int(seed),
                           int(env_index_offset), 0.0, L.INTEGRATORS[integrator],
                           {"iid": L.NOISE_IID, "shared": L.NOISE_SHARED}[noise_layout],
                           sig(*_sigmas(init_noise, self.state_dim)), sig(*_sigmas(obs_noise, self.state_dim)),
                           *((lambda m, a: (m, L.SOLVERS[solver], a))(*L.pack_env_params(env_params))),
                           L.ODE_METHODS[ode_method], int(rollout_chunk_steps))
        self._h = C.c_void_p()
        self._host_io = None
        with torch.cuda.device(self.device):
            L.check(L.lib().emei_create(C.byref(cfg), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            L.lib().emei_destroy(self._h)
            self._h = None
        # the pre-bound emei_step_host call holds the raw handle: it must not outlive it (a step_host() after
        # close() passed a dangling emei_env* into the library)
        self._host_io = None
        self._host_bufs = None

    def _live(self):
        if not self._h:
            raise L.EmeiHipError("this Engine has been closed")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state ---------------------------------------------------------------------------------
    @_on_device
    def reset(self, seed=0):
        L.check(L.lib().emei_reset(self._h, _seed64(seed), _stream()))

    def set_seed(self, seed):
        """Re-key the device reset generator (auto-reset episodes) without touching the state."""
        L.check(L.lib().emei_set_seed(self._h, _seed64(seed)))

    @_on_device
    def solver_cap_hits(self):
        """Newton solves of this engine's rollouts that ended at the iteration cap without converging (must stay 0)."""
        out = torch.zeros(1, dtype=torch.int64, device=self.device)
        L.check(L.lib().emei_get_solver_cap_hits(self._h, _ptr(out), _stream()))
        return int(out.item())

    @_on_device
    def rollout_faults(self):
        """Work items of this engine's chunked body rollouts that gave up waiting for their predecessor (must stay 0)."""
        out = torch.zeros(1, dtype=torch.int64, device=self.device)
        L.check(L.lib().emei_get_rollout_faults(self._h, _ptr(out), _stream()))
        return int(out.item())

    def set_obs_peers(self, peers, row_envs, col_offset, max_steps=None):
        """emei_set_obs_peers: from now on every rollout ALSO stores each step's observation row into the gathered buffers `peers`
        (device pointers as ints, or float32 tensors [rows, row_envs, obs_dim]; at most _lib.MAX_OBS_PEERS), this engine's envs at
        columns [col_offset, col_offset + n_envs) — the multi-GPU observation return by peer writes (sharding.PeerWriteExchange).
        An empty list switches it off.  Rollouts the staged CartPole kernel cannot serve then raise instead of skipping the peers.
        max_steps: rows of every buffer (taken from the tensors when they are tensors): a longer rollout is refused."""
        self._live()
        ptrs = [int(p.data_ptr()) if torch.is_tensor(p) else int(p) for p in peers]
        if max_steps is None and ptrs:
            if not all(torch.is_tensor(p) for p in peers):
                raise ValueError("set_obs_peers: max_steps is needed with raw pointers")
            for p in peers:
                if p.dtype != torch.float32 or not p.is_contiguous() or p.dim() != 3 or p.shape[1] != row_envs or p.shape[2] != self.obs_dim:
                    raise ValueError(f"set_obs_peers: a peer buffer is float32 [rows, {row_envs}, {self.obs_dim}], contiguous; got {p.dtype} {tuple(p.shape)}")
            max_steps = min(int(p.shape[0]) for p in peers)
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        L.check(L.lib().emei_set_obs_peers(self._h, len(ptrs), arr, int(row_envs), int(col_offset), int(max_steps or 0)))
        self._peer_refs = [p for p in peers if torch.is_tensor(p)]  # keep local targets alive while they are written to

    def last_kernel(self):
        """enum emei_kernel_id of the kernel the last step / rollout launched (_lib.kernel_name)."""
        self._live()
        return int(L.lib().emei_last_rollout_kernel(self._h))

    @_on_device
    def set_state(self, state, reset_counters=True):
        st = torch.as_tensor(state, dtype=torch.float64, device=self.device).contiguous()
        if tuple(st.shape) != (self.n_envs, self.state_dim):
            raise ValueError(f"state shape {tuple(st.shape)} != {(self.n_envs, self.state_dim)}")
        L.check(L.lib().emei_set_state(self._h, _ptr(st), int(bool(reset_counters)), _stream()))
        torch.cuda.current_stream().synchronize()  # `st` may be a temporary

    @_on_device
    def get_state(self):
        out = torch.empty((self.n_envs, self.state_dim), dtype=torch.float64, device=self.device)
        L.check(L.lib().emei_get_state(self._h, _ptr(out), _stream()))
        return out

    @_on_device
    def get_obs(self):
        out = torch.empty((self.n_envs, self.obs_dim), dtype=torch.float64, device=self.device)
        L.check(L.lib().emei_get_obs(self._h, _ptr(out), _stream()))
        return out

    @_on_device
    def freeze(self):
        L.check(L.lib().emei_freeze(self._h, _stream()))

    @_on_device
    def unfreeze(self):
        L.check(L.lib().emei_unfreeze(self._h, _stream()))

    @property
    def _act_tail(self):
        """the trailing dimensions of an action array: (act_dim,) for act_dim > 1, nothing otherwise"""
        return (self.act_dim,) if self.act_dim > 1 else ()

    def _workspace(self, attr, size_fn, K):
        """the cached device workspace `attr` of a plan call, at least size_fn(n_envs, K) bytes: grow-only (a captured graph keeps
        using the tensor it was captured with), float64 elements (8-byte aligned records), one per method"""
        need = int(size_fn(self.n_envs, K))
        if need < 0:
            L.check(need)
        ws = getattr(self, attr, None)
        if ws is None or ws.numel() * 8 < need:
            ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
            setattr(self, attr, ws)
        return ws

    # -- hot path ------------------------------------------------------------------------------
    def _check_actions(self, actions, lead):
        return self._check_actions_n(actions, lead, self.n_envs)

    def _check_actions_n(self, actions, lead, n):
        """actions must be lead + [n(, act_dim)], contiguous, on the engine's device -> enum emei_action_dtype"""
        if not isinstance(actions, torch.Tensor) or actions.device != self.device:
            raise ValueError("actions must be a tensor on the engine's device")
        if actions.dtype not in _ACT_DTYPES:
            raise ValueError(f"unsupported action dtype {actions.dtype}")
        want = lead + ((n,) if self.act_dim <= 1 else (n, self.act_dim))
        shape = tuple(actions.shape)
        if shape != want and not (self.act_dim == 1 and shape == lead + (n, 1)):
            raise ValueError(f"actions shape {shape} != {want}")
        if not actions.is_contiguous():
            raise ValueError("actions must be contiguous")
        return _ACT_DTYPES[actions.dtype]

    def _check_outputs(self, out, lead):
        """Caller-supplied output buffers go to the ABI as raw pointers (it has no size arguments): a wrong shape, dtype,
        device or stride would be a silent out-of-bounds device write.  Checked on EVERY call and nothing is retained: a
        tensor can be resize_()d / set_() between calls, and holding callers' buffers alive would pin their device memory."""
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise ValueError("out must be (obs, reward, done)")
        n = self.n_envs
        for t, shape, dtype, name in ((out[0], lead + (n, self.obs_dim), torch.float32, "obs"),
                                      (out[1], lead + (n,), torch.float32, "reward"), (out[2], lead + (n,), torch.uint8, "done")):
            if not isinstance(t, torch.Tensor) or t.device != self.device:
                raise ValueError(f"out: {name} must be a tensor on {self.device}")
            if t.shape != shape or t.dtype != dtype:
                raise ValueError(f"out: {name} is {tuple(t.shape)} {t.dtype}, expected {shape} {dtype}")
            if not t.is_contiguous():
                raise ValueError(f"out: {name} must be contiguous")
        return out

    @_on_device
    def step(self, actions, auto_reset=False, out=None):
        """-> obs [N,obs_dim] f32, reward [N] f32, done [N] u8 (bit0 terminal, bit1 truncated)."""
        dt = self._check_actions(actions, ())
        obs, rew, done = self._check_outputs(out, ()) if out is not None else self.alloc_outputs(None)
        L.check(L.lib().emei_step(self._h, _ptr(actions), dt, _ptr(obs), _ptr(rew), _ptr(done),
                                  L.FLAG_AUTO_RESET if auto_reset else 0, _stream()))
        return obs, rew, done

    def step_host(self, action, auto_reset=False):
        """The gym-style single-env call (`env.step(a)` of base_control.py:61-83 with host values in and out) through
        emei_step_host: actions and results live in pinned host memory that the kernels address directly; for one env of the
        4-state family a step is ONE launch whose last store is a completion word the library polls (no copy, no stream
        synchronisation), otherwise step + emei_get_obs + one synchronisation.
        action: array-like [N(,act_dim)] -> (obs float64 [N,obs_dim] of the post-step state, obs float32
        [N,obs_dim] as emitted by the step (pre auto-reset), reward float32 [N], done uint8 [N]) as NumPy
        views of the pinned buffers (valid until the next call)."""
        io = self._host_io
        if io is None:
            self._live()
            io = self._host_io = self._make_host_io()
        act_np, obs64_np, obs32_np, rew_np, done_np, call, flag_auto = io
        act_np[...] = action
        if torch.cuda.current_device() != self.device.index:
            with torch.cuda.device(self.device):
                rc = call(flag_auto if auto_reset else 0, _stream_handle(self.device.index))
        else:
            rc = call(flag_auto if auto_reset else 0, _stream_handle(self.device.index))
        if rc:
            L.check(rc)
        return obs64_np, obs32_np, rew_np, done_np

    def _make_host_io(self):
        import functools

        pin = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)
        ashape = (self.n_envs,) if self.act_dim <= 1 else (self.n_envs, self.act_dim)
        act = pin(ashape, torch.int64 if self.act_dim == 0 else torch.float32)
        bufs = (act, pin((self.n_envs, self.obs_dim), torch.float64), pin((self.n_envs, self.obs_dim), torch.float32),
                pin((self.n_envs,), torch.float32), pin((self.n_envs,), torch.uint8))
        self._host_bufs = bufs  # keeps the pinned allocations alive
        # the pointers never change: bind them once (a ctypes call costs per converted argument)
        call = functools.partial(L.lib().emei_step_host, self._h, _ptr(act), _ACT_DTYPES[act.dtype], _ptr(bufs[1]), _ptr(bufs[2]),
                                 _ptr(bufs[3]), _ptr(bufs[4]))
        return tuple(b.numpy() for b in bufs) + (call, L.FLAG_AUTO_RESET)

    @_on_device
    def rollout(self, actions, auto_reset=False, out=None):
        """actions [T,N(,act_dim)] -> obs [T,N,obs_dim] f32, reward [T,N] f32, done [T,N] u8; one launch."""
        T = int(actions.shape[0])
        dt = self._check_actions(actions, (T,))
        obs, rew, done = self._check_outputs(out, (T,)) if out is not None else self.alloc_outputs(T)
        L.check(L.lib().emei_rollout(self._h, T, _ptr(actions), dt, _ptr(obs), _ptr(rew), _ptr(done),
                                     L.FLAG_AUTO_RESET if auto_reset else 0, _stream()))
        return obs, rew, done

    @_on_device
    def rollout_policy(self, T, policy, auto_reset=False, out=None, noise=None):
        """T closed-loop steps under a feedback policy in one launch (emei_rollout_policy): per step the policy (policy.MLPPolicy)
        is evaluated inside the kernel on the observation the env holds — get_obs() rounded to float32 at first, then the row each
        step emits, or episode_init_obs of the new episode after an auto-reset — and the envs take step(action, auto_reset): bit for
        bit what that loop computes with policy(obs) as the callable (out="clip" and the discrete envs; out="tanh" up to the
        device's tanh), state, counters and compact_done() included.
        -> (actions [T, N(, act_dim)] int64 / float32, obs [T, N, obs_dim] f32, reward [T, N] f32, done [T, N] u8).
        out: (obs, reward, done) as rollout's.
        noise: a policy.PolicyNoise — exploration noise drawn inside the kernel (emei_rollout_policy_noisy): Gaussian on the continuous
        envs, epsilon-greedy on the discrete ones; step t draws under the key noise.seed + t, and the loop that calls
        policy(obs, noise, t) gives the same actions.  None: the deterministic launch.
        A policy.DeepMLPPolicy (two hidden layers) goes to emei_rollout_policy_deep, with or without noise."""
        T = int(T)
        if T < 1:
            raise ValueError(f"n_steps={T} must be >= 1")
        from .policy import DeepMLPPolicy, MLPPolicy, PolicyNoise

        if not isinstance(policy, MLPPolicy):
            raise TypeError("rollout_policy takes an emei_amd.MLPPolicy (any other callable acts through the per-step loop: step())")
        policy.bind(self)
        obs, rew, done = self._check_outputs(out, (T,)) if out is not None else self.alloc_outputs(T)
        dtype = torch.int64 if self.act_dim == 0 else torch.float32
        act = torch.empty((T, self.n_envs) + self._act_tail, dtype=dtype, device=self.device)
        ps = policy.struct()
        flags = L.FLAG_AUTO_RESET if auto_reset else 0
        if noise is not None and not isinstance(noise, PolicyNoise):
            raise TypeError("noise= takes an emei_amd.PolicyNoise")
        if isinstance(policy, DeepMLPPolicy):
            ns = None if noise is None else noise.bind(self).struct(policy.hidden2)
            L.check(L.lib().emei_rollout_policy_deep(self._h, T, C.byref(ps), None if ns is None else C.byref(ns), _ptr(act),
                                                     _ACT_DTYPES[dtype], _ptr(obs), _ptr(rew), _ptr(done), flags, _stream()))
            return act, obs, rew, done
        if noise is None:
            L.check(L.lib().emei_rollout_policy(self._h, T, C.byref(ps), _ptr(act), _ACT_DTYPES[dtype], _ptr(obs), _ptr(rew), _ptr(done),
                                                flags, _stream()))
            return act, obs, rew, done
        ns = noise.bind(self).struct(policy.hidden if policy.hidden else policy.obs_dim)
        L.check(L.lib().emei_rollout_policy_noisy(self._h, T, C.byref(ps), C.byref(ns), _ptr(act), _ACT_DTYPES[dtype], _ptr(obs), _ptr(rew),
                                                  _ptr(done), flags, _stream()))
        return act, obs, rew, done

    @_on_device
    def evaluate_sequences(self, actions, discount=1.0, start_state=None, final_obs=False, value=None):
        """Score K candidate action sequences per env from the current state (or `start_state`) in one launch, for planners
        (emei_evaluate_sequences).  The handle's state, counters and snapshot are left as they are.
        actions [H, N, K(, act_dim)] on the engine's device; start_state None or [N, state_dim] (float64 rows of set_state).
        -> (returns float64 [N, K]: sum of discount^t * reward_t up to the first terminal step, included; lengths int32 [N, K]:
        that step + 1, or H; [final_obs float32 [N, K, obs_dim]: the observation of the last counted step])
        value= (a policy.DeepValueFunction) adds a TERMINAL VALUE (emei_evaluate_sequences_value): every candidate that set no terminal
        bit in its H steps gets discount^H * float64(V(final obs)) on top of its return; one that terminated gets nothing, at the last
        step included (its length is H too).  Lengths and final_obs do not change."""
        vs = self._plan_value(value, "evaluate_sequences")
        if not isinstance(actions, torch.Tensor) or actions.dim() < 3:
            raise ValueError("actions must be a tensor [H, N, K(, act_dim)] on the engine's device")
        H, K = int(actions.shape[0]), int(actions.shape[2])
        if actions.shape[1] != self.n_envs:
            raise ValueError(f"actions shape {tuple(actions.shape)}: dimension 1 must be n_envs={self.n_envs}")
        if not actions.is_contiguous():
            raise ValueError("actions must be contiguous")
        # [H, N, K(, act_dim)] is the rollout layout [H, N * K(, act_dim)] of N * K envs
        flat = actions.view((H, self.n_envs * K) + tuple(actions.shape[3:]))
        dt = self._check_actions_n(flat, (H,), self.n_envs * K)
        st = self._start_rows(start_state)
        ret = torch.empty((self.n_envs, K), dtype=torch.float64, device=self.device)
        length = torch.empty((self.n_envs, K), dtype=torch.int32, device=self.device)
        fo = torch.empty((self.n_envs, K, self.obs_dim), dtype=torch.float32, device=self.device) if final_obs else None
        if vs is None:
            L.check(L.lib().emei_evaluate_sequences(self._h, H, K, _ptr(flat), dt, float(discount), _ptr(st), _ptr(ret), _ptr(length),
                                                    _ptr(fo), _stream()))
        else:
            L.check(L.lib().emei_evaluate_sequences_value(self._h, H, K, _ptr(flat), dt, float(discount), C.byref(vs), _ptr(st), _ptr(ret),
                                                          _ptr(length), _ptr(fo), _stream()))
        return (ret, length, fo) if final_obs else (ret, length)

    @_on_device
    def evaluate_policies(self, pop, H, discount=1.0, start_state=None, final_obs=False):
        """Score a population of P feedback policies, each on every env, from the current state (or `start_state`) in one launch, for
        policy search (emei_evaluate_policies): pair (p, i) runs policy p closed-loop for H steps from env i's start state, as
        rollout_policy(H, pop[p], auto_reset=False) would, and is scored as evaluate_sequences scores.  The handle's state, counters
        and snapshot are left as they are.  pop: a policy.PolicyPopulation, or one MLPPolicy as a population of one; a
        policy.DeepPolicyPopulation or one DeepMLPPolicy (two hidden layers) goes to emei_evaluate_policies_deep.
        -> (returns float64 [P, N], lengths int32 [P, N][, final_obs float32 [P, N, obs_dim]: the observation of the last counted step])"""
        from .policy import DeepMLPPolicy, DeepPolicyPopulation, MLPPolicy, PolicyPopulation

        if isinstance(pop, DeepMLPPolicy):
            pop = DeepPolicyPopulation.from_policies([pop])
        elif isinstance(pop, MLPPolicy):
            pop = PolicyPopulation.from_policies([pop])
        if not isinstance(pop, (PolicyPopulation, DeepPolicyPopulation)):
            raise TypeError("evaluate_policies takes an emei_amd.PolicyPopulation / DeepPolicyPopulation or an emei_amd.MLPPolicy")
        H = int(H)
        if H < 1:
            raise ValueError(f"horizon={H} must be >= 1")
        pop.bind(self)
        P = len(pop)
        st = self._start_rows(start_state)
        ret = torch.empty((P, self.n_envs), dtype=torch.float64, device=self.device)
        length = torch.empty((P, self.n_envs), dtype=torch.int32, device=self.device)
        fo = torch.empty((P, self.n_envs, self.obs_dim), dtype=torch.float32, device=self.device) if final_obs else None
        ps = pop.struct()
        entry = L.lib().emei_evaluate_policies_deep if isinstance(pop, DeepPolicyPopulation) else L.lib().emei_evaluate_policies
        L.check(entry(self._h, H, P, C.byref(ps), float(discount), _ptr(st), _ptr(ret), _ptr(length), _ptr(fo), _stream()))
        return (ret, length, fo) if final_obs else (ret, length)

    def _plan_value(self, value, who):
        """the checked terminal value of the open-loop plan calls (evaluate_sequences, plan_shooting, plan_mppi, plan_cem): None, or
        struct emei_policy_deep over a policy.DeepValueFunction bound to this engine as plan_policy binds it.  Needs no handle."""
        if value is None:
            return None
        from .policy import DeepValueFunction

        if not isinstance(value, DeepValueFunction):
            raise TypeError(f"{who} takes an emei_amd.DeepValueFunction as value= (the terminal value network), or None")
        return value.bind(self).struct()

    def _start_rows(self, start_state):
        """validated start_state of the plan calls: None, or contiguous float64 rows [N, state_dim] on the engine's device"""
        if start_state is None:
            return None
        st = torch.as_tensor(start_state, device=self.device)
        if st.dtype != torch.float64 or tuple(st.shape) != (self.n_envs, self.state_dim) or not st.is_contiguous():
            raise ValueError(f"start_state must be a contiguous float64 tensor {(self.n_envs, self.state_dim)} on {self.device}; "
                             f"got {st.dtype} {tuple(st.shape)}")
        return st

    # -- random-shooting planning: candidates drawn and arg-maxed on the device (emei_plan_shooting) -------------
    def _candidate_args(self, H, K, nominal, sigma, dtype):
        """validated (nominal tensor or None, sigma, torch dtype) of sample_candidates / plan_shooting: the ABI takes raw pointers"""
        H, K = int(H), int(K)
        if H < 1 or K < 1:
            raise ValueError(f"horizon={H} and n_candidates={K} must be >= 1")
        if dtype is None:
            dtype = torch.int64 if self.act_dim == 0 else torch.float32  # what step() takes by default
        if dtype not in _ACT_DTYPES or (dtype == torch.float32) != (self.act_dim > 0):
            raise ValueError(f"action dtype {dtype}: uint8 / int32 / int64 for the discrete envs, float32 for the continuous ones")
        if nominal is not None:
            want = (H, self.n_envs) if self.act_dim == 0 else (H, self.n_envs, self.act_dim)
            if not isinstance(nominal, torch.Tensor) or nominal.device != self.device:
                raise ValueError("nominal must be a tensor on the engine's device")
            ok_shape = tuple(nominal.shape) == want or (self.act_dim == 1 and tuple(nominal.shape) == (H, self.n_envs))
            if nominal.dtype != torch.float32 or not ok_shape or not nominal.is_contiguous():
                raise ValueError(f"nominal must be a contiguous float32 tensor {want}; got {nominal.dtype} {tuple(nominal.shape)}")
            if self.act_dim > 0 and sigma is None:
                raise ValueError("nominal on a continuous env needs sigma")
        return H, K, nominal, float(0.0 if sigma is None else sigma), dtype

    def _sigma_map(self, nominal, sigma):
        """validated per-entry sigma of sample_candidates / plan_cem: a float32 tensor of nominal's shape (continuous envs only)"""
        if self.act_dim == 0:
            raise ValueError("a discrete env takes no sigma tensor")
        if nominal is None:
            raise ValueError("a sigma tensor needs a nominal")
        if sigma.device != self.device or sigma.dtype != torch.float32 or not sigma.is_contiguous() \
                or sigma.numel() != nominal.numel() or sigma.dim() != nominal.dim():
            raise ValueError(f"a sigma tensor must be a contiguous float32 tensor of nominal's shape {tuple(nominal.shape)} on "
                             f"{self.device}; got {sigma.dtype} {tuple(sigma.shape)}")
        return sigma

    @_on_device
    def sample_candidates(self, H, K, seed, nominal=None, sigma=None, dtype=None):
        """The candidate sequences plan_shooting(H, K, seed, nominal=, sigma=) draws, written out (emei_sample_candidates):
        [H, N, K(, act_dim)] in evaluate_sequences' layout.  nominal None: fair coin flips / uniform on the ctrlrange; else float32
        [H, N] Bernoulli probabilities (discrete) or [H, N, act_dim] means of clipped Gaussians with `sigma` (continuous).
        sigma: a float, or a float32 tensor of nominal's shape with one sigma per entry (emei_sample_candidates_sigma: what
        plan_cem(sigma=tensor) draws; an entry of 0 gives the clipped mean).
        dtype: uint8 / int32 / int64 (discrete; the default int64) or float32."""
        is_map = isinstance(sigma, torch.Tensor)
        H, K, nominal, scalar, dtype = self._candidate_args(H, K, nominal, 1.0 if is_map else sigma, dtype)
        if is_map:
            fn, sig = L.lib().emei_sample_candidates_sigma, _ptr(self._sigma_map(nominal, sigma))
        else:
            fn, sig = L.lib().emei_sample_candidates, scalar
        out = torch.empty((H, self.n_envs, K) + self._act_tail, dtype=dtype, device=self.device)
        L.check(fn(self._h, H, K, _seed64(seed), _ptr(nominal), sig, _ptr(out), _ACT_DTYPES[dtype], _stream()))
        return out

    @_on_device
    def plan_shooting(self, H, K, seed, discount=1.0, nominal=None, sigma=None, start_state=None, sequence=False, length=False,
                      dtype=None, value=None):
        """Random shooting in two launches (emei_plan_shooting): K candidate sequences of H steps per env are drawn in the lanes
        that score them from the current state (or `start_state` [N, state_dim] float64) and arg-maxed on the device.
        -> (best_action [N(, act_dim)], best_return float64 [N], best_index int32 [N][, best_sequence [H, N(, act_dim)]]
        [, best_length int32 [N]]): the first maximum of evaluate_sequences(sample_candidates(...)) per env, NaN returns below
        everything.  The handle is left as it is.  Arguments as sample_candidates.
        value= (a policy.DeepValueFunction): the candidates are scored as evaluate_sequences(..., value=) scores them
        (emei_plan_shooting_value), and the winner, its return and its length are those of the bootstrapped returns."""
        vs = self._plan_value(value, "plan_shooting")
        H, K, nominal, sigma, dtype = self._candidate_args(H, K, nominal, sigma, dtype)
        st = self._start_rows(start_state)
        if vs is None:
            ws = self._workspace("_plan_ws", L.lib().emei_plan_shooting_workspace_bytes, K)
        else:
            ws = self._workspace("_plan_value_ws", L.lib().emei_plan_value_workspace_bytes, K)
        act = torch.empty((self.n_envs,) + self._act_tail, dtype=dtype, device=self.device)
        seq = torch.empty((H, self.n_envs) + self._act_tail, dtype=dtype, device=self.device) if sequence else None
        ret = torch.empty(self.n_envs, dtype=torch.float64, device=self.device)
        idx = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        ln = torch.empty(self.n_envs, dtype=torch.int32, device=self.device) if length else None
        head = (self._h, H, K, _seed64(seed), _ptr(nominal), sigma, float(discount))
        tail = (_ptr(st), _ptr(ws), _ptr(act), _ACT_DTYPES[dtype], _ptr(seq), _ptr(ret), _ptr(idx), _ptr(ln), _stream())
        if vs is None:
            L.check(L.lib().emei_plan_shooting(*head, *tail))
        else:
            L.check(L.lib().emei_plan_shooting_value(*head, C.byref(vs), *tail))
        return (act, ret, idx) + ((seq,) if sequence else ()) + ((ln,) if length else ())

    @_on_device
    def plan_mppi(self, H, K, seed, temperature, discount=1.0, nominal=None, sigma=None, start_state=None, out=None, ess=False,
                  value=None):
        """The MPPI update of a nominal sequence in two launches (emei_plan_mppi): the K candidates per env that
        plan_shooting(H, K, seed, nominal=, sigma=) scores are scored the same way, weighted by exp((return - best) / temperature)
        (NaN returns weigh 0, ties with the best 1) and averaged — the candidates redrawn on the device, never stored.
        -> (nominal_out float32 [H, N(, act_dim)], best_return float64 [N], best_index int32 [N][, ess float64 [N]]): the weighted
        mean (a mean inside the ctrlrange, or a Bernoulli probability for the discrete envs: the next call's `nominal`), plan_shooting's
        winner bit for bit, and the effective sample size (sum w)^2 / sum w^2.  out: a float32 tensor of nominal_out's shape to write
        into; it may be `nominal` itself (in place).  The handle is left as it is.  Other arguments as sample_candidates.
        value= (a policy.DeepValueFunction): MPPI with a terminal value (emei_plan_mppi_value) — the weights, the mean, the winner and
        the ess use the returns evaluate_sequences(..., value=) gives; the winner is plan_shooting(..., value=)'s bit for bit."""
        vs = self._plan_value(value, "plan_mppi")
        H, K, nominal, sigma, _ = self._candidate_args(H, K, nominal, sigma, None)
        temperature = float(temperature)
        st = self._start_rows(start_state)
        shape = (H, self.n_envs) + self._act_tail
        if out is None:
            out = torch.empty(shape if nominal is None else tuple(nominal.shape), dtype=torch.float32, device=self.device)
        else:
            self._check_plan_out("out", out, shape, nominal, "nominal")
        if vs is None:
            ws = self._workspace("_mppi_ws", L.lib().emei_plan_mppi_workspace_bytes, K)
        else:
            ws = self._workspace("_plan_value_ws", L.lib().emei_plan_value_workspace_bytes, K)
        ret = torch.empty(self.n_envs, dtype=torch.float64, device=self.device)
        idx = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        es = torch.empty(self.n_envs, dtype=torch.float64, device=self.device) if ess else None
        head = (self._h, H, K, _seed64(seed), _ptr(nominal), sigma, float(discount))
        tail = (temperature, _ptr(st), _ptr(ws), _ptr(out), _ptr(ret), _ptr(idx), _ptr(es), _stream())
        if vs is None:
            L.check(L.lib().emei_plan_mppi(*head, *tail))
        else:
            L.check(L.lib().emei_plan_mppi_value(*head, C.byref(vs), *tail))
        return (out, ret, idx) + ((es,) if ess else ())

    # -- planning around a feedback policy (emei_plan_policy) ---------------------------------------------------
    def _plan_policy_args(self, H, K, policy, noise, discount, temperature):
        """_plan_policy_checked for the one-layer calls (plan_policy, mpc_policy), which have no value network"""
        H, K, ps, ns, _, discount, temperature = _plan_policy_checked(self, H, K, policy, noise, None, discount, temperature, False)
        return H, K, ps, ns, discount, temperature

    def _plan_policy_deep_args(self, H, K, policy, noise, value, discount, temperature):
        return _plan_policy_checked(self, H, K, policy, noise, value, discount, temperature, True)

    @_on_device
    def plan_policy(self, H, K, policy, noise, discount=1.0, temperature=None, start_state=None, returns=False, length=False, ess=False,
                    value=None):
        """Shooting and MPPI around a feedback policy in two launches (emei_plan_policy): per env, K closed-loop rollouts of `policy`
        (a policy.MLPPolicy) for H steps from the current state (or `start_state` [N, state_dim] float64), candidate k under the
        exploration noise of `noise` (a policy.PolicyNoise) drawn in the lanes with k in the counter word — candidate 0 takes no noise:
        it is the policy itself — scored as evaluate_sequences scores, and arg-maxed on the device.  The loop "observe,
        policy(obs, noise, t, candidate=k) (policy(obs) for k = 0), step" takes candidate k's actions.
        -> (best_action [N(, act_dim)] int64 / float32: the winner's action at t = 0, best_return float64 [N], best_index int32 [N]
        [, mean_action float32 [N(, act_dim)]: the mean of the K first actions weighted by exp((return - best) / temperature), as
        plan_mppi weighs (on a discrete env the weighted share of action 1) — with a temperature]
        [, returns float64 [N, K]][, best_length int32 [N]][, ess float64 [N]: (sum w)^2 / sum w^2, needs a temperature]).
        The handle is left as it is.
        A policy.DeepMLPPolicy (two hidden layers, e.g. a 256-256 actor) goes to emei_plan_policy_deep: the same call, candidates,
        noise streams and outputs on kernels of their own.  With it, value= (a policy.DeepValueFunction) adds a TERMINAL VALUE: every
        candidate that never terminated in its H steps gets discount^H * float64(V(final obs)) on top of its return (a candidate that
        terminated gets nothing), and the arg-max, the weights, the mean, `returns` and the ess all use the bootstrapped returns —
        the planner of MBOP, LOOP, POLO and TD-MPC.  value= with a one-layer MLPPolicy is refused."""
        from .policy import DeepMLPPolicy

        deep = isinstance(policy, DeepMLPPolicy)
        if value is not None and not deep:
            raise ValueError("plan_policy: value= (the terminal value) comes with the two-hidden-layer call: pass a DeepMLPPolicy (a "
                             "one-layer policy embeds in one exactly: include/emei_hip.h, emei_rollout_policy_deep)")
        H, K, ps, ns, vs, discount, temperature = _plan_policy_checked(self, H, K, policy, noise, value, discount, temperature, deep)
        if ess and temperature is None:
            raise ValueError("ess=True needs a temperature")
        st = self._start_rows(start_state)
        ws = self._workspace("_plan_policy_ws", L.lib().emei_plan_policy_workspace_bytes, K)
        dtype = torch.int64 if self.act_dim == 0 else torch.float32
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        act = new((self.n_envs,) + self._act_tail, dtype)
        mean = new((self.n_envs,) + self._act_tail, torch.float32) if temperature is not None else None
        ret, idx = new(self.n_envs, torch.float64), new(self.n_envs, torch.int32)
        ln = new(self.n_envs, torch.int32) if length else None
        rets = new((self.n_envs, K), torch.float64) if returns else None
        es = new(self.n_envs, torch.float64) if ess else None
        tail = (discount, 1.0 if temperature is None else temperature, _ptr(st), _ptr(ws), _ptr(act), _ACT_DTYPES[dtype], _ptr(mean),
                _ptr(ret), _ptr(idx), _ptr(ln), _ptr(rets), _ptr(es), _stream())
        if deep:
            L.check(L.lib().emei_plan_policy_deep(self._h, H, K, C.byref(ps), C.byref(ns), C.byref(vs) if vs is not None else None, *tail))
        else:
            L.check(L.lib().emei_plan_policy(self._h, H, K, C.byref(ps), C.byref(ns), *tail))
        return (act, ret, idx) + ((mean,) if mean is not None else ()) + ((rets,) if returns else ()) + ((ln,) if length else ()) \
            + ((es,) if ess else ())

    def _mpc_nominal_defaults(self, refill, clamp):
        """(refill, lo, hi) of mpc_mppi / mpc_cem with their defaults: refill 0.5 (discrete) / 0.0 (continuous), the clamp (0.05, 0.95)
        on the discrete envs and the ctrlrange on the continuous ones"""
        if refill is None:
            refill = 0.5 if self.act_dim == 0 else 0.0
        if clamp is None:
            clamp = (0.05, 0.95) if self.act_dim == 0 else _CTRL_RANGE.get(self.env_name, (-1.0, 1.0))
        return refill, float(clamp[0]), float(clamp[1])

    def _mpc_outputs(self, T, out, dtype, diagnostics):
        """what a fused controller fills: (actions [T, N(, act_dim)] of `dtype`, obs, reward, done — `out`, checked, or new ones, as
        rollout's — and a list with one [T, N] tensor per dtype of `diagnostics`, None for a None)"""
        obs, rew, done = self._check_outputs(out, (T,)) if out is not None else self.alloc_outputs(T)
        act = torch.empty((T, self.n_envs) + self._act_tail, dtype=dtype, device=self.device)
        diag = [None if dt is None else torch.empty((T, self.n_envs), dtype=dt, device=self.device) for dt in diagnostics]
        return act, obs, rew, done, diag

    @_on_device
    def mpc_mppi(self, T, H, K, seed, temperature, nominal, discount=1.0, sigma=None, refill=None, clamp=None, auto_reset=False,
                 out=None, diagnostics=False):
        """T control steps of receding-horizon MPPI in one launch (emei_mpc_mppi; the 4-state envs and the InvertedDoublePendulum
        without observation noise, each on kernels of its own): per step the nominal is clamped to `clamp`, updated as
        plan_mppi(H, K, seed + t, temperature, nominal=nominal, out=nominal) updates it, its first entry is the action (discrete envs: entry >= 0.5), the envs take step(action, auto_reset), and the
        nominal is shifted by one step with `refill` behind it (an env that was reset: `refill` everywhere) — bit for bit what
        that loop of plan_mppi and step computes, state, counters and compact_done() included.
        nominal: float32 [H, N(, act_dim)] on the engine's device, updated IN PLACE (ready for the next call: T = a + b steps equal
        a call with (a, seed) and one with (b, seed + a)).  refill: default 0.5 (discrete) / 0.0 (continuous).  clamp: (lo, hi),
        default (0.05, 0.95) on the discrete envs and the ctrlrange on the continuous ones (InvertedPendulum +-3,
        InvertedDoublePendulum +-1).  out: (obs, reward, done) as rollout's.
        -> (actions [T, N(, act_dim)] int64 / float32, obs [T, N, obs_dim] f32, reward [T, N] f32, done [T, N] u8
        [, plan_return float64 [T, N], ess float64 [T, N]]: every step's best candidate return and effective sample size)."""
        T = int(T)
        if T < 1:
            raise ValueError(f"n_steps={T} must be >= 1")
        if nominal is None:
            raise ValueError("mpc_mppi needs a nominal tensor (it is updated in place)")
        H, K, nominal, sigma, dtype = self._candidate_args(H, K, nominal, sigma, None)
        refill, lo, hi = self._mpc_nominal_defaults(refill, clamp)
        act, obs, rew, done, (pr, es) = self._mpc_outputs(T, out, dtype, (torch.float64,) * 2 if diagnostics else (None,) * 2)
        ws = self._workspace("_mpc_ws", L.lib().emei_mpc_mppi_workspace_bytes, K)
        L.check(L.lib().emei_mpc_mppi(self._h, T, H, K, _seed64(seed), _ptr(nominal), sigma, float(discount), float(temperature),
                                      float(refill), lo, hi, _ptr(ws), _ptr(act), _ACT_DTYPES[dtype], _ptr(obs), _ptr(rew), _ptr(done),
                                      _ptr(pr), _ptr(es), L.FLAG_AUTO_RESET if auto_reset else 0, _stream()))
        return (act, obs, rew, done) + ((pr, es) if diagnostics else ())

    @_on_device
    def mpc_cem(self, T, H, K, n_elites, seed, nominal, iterations=1, sigma=None, sigma_min=0.0, discount=1.0, refill=None, clamp=None,
                auto_reset=False, out=None, diagnostics=False):
        """T control steps of receding-horizon CEM in one launch (emei_mpc_cem; the envs mpc_mppi serves): per step,
        `iterations` times, the mean is clamped to `clamp` and refitted as plan_cem(H, K, n_elites, seed + t * iterations + j,
        nominal=mean, sigma=std, out=mean, out_sigma=std) refits it — std a per-entry tensor that starts every control step at
        `sigma` and is floored at `sigma_min` after every refit (continuous envs; the discrete ones have none) — then the mean's first
        entry is the action (discrete envs: entry >= 0.5), the envs take step(action, auto_reset), and the mean is shifted by one
        step with `refill` behind it (an env that was reset: `refill` everywhere) — bit for bit what that loop of plan_cem and step
        computes, state, counters and compact_done() included.
        nominal: float32 [H, N(, act_dim)] on the engine's device, the mean, updated IN PLACE (T = a + b steps equal a call with
        (a, seed) and one with (b, seed + a * iterations)).  Defaults of refill, clamp and out as mpc_mppi's.
        -> (actions [T, N(, act_dim)] int64 / float32, obs [T, N, obs_dim] f32, reward [T, N] f32, done [T, N] u8
        [, plan_return float64 [T, N], elite_return float64 [T, N]]: the best candidate return and the admission threshold of every
        step's last iteration)."""
        T, n_elites, iterations = int(T), int(n_elites), int(iterations)
        if T < 1:
            raise ValueError(f"n_steps={T} must be >= 1")
        if nominal is None:
            raise ValueError("mpc_cem needs a nominal tensor (it is updated in place)")
        H, K, nominal, sigma, dtype = self._candidate_args(H, K, nominal, sigma, None)
        if not 1 <= n_elites <= K:
            raise ValueError(f"n_elites={n_elites} is outside [1, n_candidates={K}]")
        if iterations < 1:
            raise ValueError(f"iterations={iterations} must be >= 1")
        refill, lo, hi = self._mpc_nominal_defaults(refill, clamp)
        act, obs, rew, done, (pr, er) = self._mpc_outputs(T, out, dtype, (torch.float64,) * 2 if diagnostics else (None,) * 2)
        ws = self._workspace("_mpc_cem_ws", L.lib().emei_mpc_cem_workspace_bytes, K)
        L.check(L.lib().emei_mpc_cem(self._h, T, H, K, n_elites, iterations, _seed64(seed), _ptr(nominal), sigma, float(sigma_min),
                                     float(discount), float(refill), lo, hi, _ptr(ws), _ptr(act), _ACT_DTYPES[dtype], _ptr(obs), _ptr(rew),
                                     _ptr(done), _ptr(pr), _ptr(er), L.FLAG_AUTO_RESET if auto_reset else 0, _stream()))
        return (act, obs, rew, done) + ((pr, er) if diagnostics else ())

    @_on_device
    def mpc_policy(self, T, H, K, policy, noise, act="best", temperature=None, seed_stride=None, discount=1.0, auto_reset=False,
                   out=None, diagnostics=False):
        """T control steps of policy-guided MPC in one launch (emei_mpc_policy; the envs mpc_mppi serves): per step t,
        plan_policy(H, K, policy, noise_t, discount, temperature) from the current states with noise_t = `noise` under the seed
        noise.seed + t * seed_stride, then the action — act="best": the best candidate's first action; act="mean": the
        return-weighted mean of the K first actions (discrete envs: mean >= 0.5), which needs a temperature — and
        step(action, auto_reset): bit for bit what that loop of plan_policy and step computes, state, counters and compact_done()
        included.  policy: a policy.MLPPolicy with one hidden layer or none (a DeepMLPPolicy is not served by this call: plan_policy
        serves it); noise: a policy.PolicyNoise.  seed_stride: default H, so that the noise keys of consecutive control steps do not
        overlap; T = a + b steps equal a call with (a, noise) and one with (b, the noise under seed + a * seed_stride).
        out: (obs, reward, done) as rollout's.
        -> (actions [T, N(, act_dim)] int64 / float32, obs [T, N, obs_dim] f32, reward [T, N] f32, done [T, N] u8
        [, plan_return float64 [T, N], plan_index int32 [T, N][, ess float64 [T, N]: with a temperature]])."""
        from .policy import DeepMLPPolicy

        T = int(T)
        if T < 1:
            raise ValueError(f"n_steps={T} must be >= 1")
        if isinstance(policy, DeepMLPPolicy):
            raise NotImplementedError("mpc_policy: the two-hidden-layer network (DeepMLPPolicy) is not served by the fused controller; "
                                      "plan_policy serves it (one plan_policy and one step per control step)")
        if act not in ("best", "mean"):
            raise ValueError(f"act={act!r}: 'best' or 'mean'")
        if act == "mean" and temperature is None:
            raise ValueError("act='mean' needs a temperature")
        H, K, ps, ns, discount, temperature = self._plan_policy_args(H, K, policy, noise, discount, temperature)
        stride = H if seed_stride is None else int(seed_stride)
        dtype = torch.int64 if self.act_dim == 0 else torch.float32
        diag = (torch.float64, torch.int32, torch.float64 if temperature is not None else None) if diagnostics else (None,) * 3
        actions, obs, rew, done, (pr, pi, es) = self._mpc_outputs(T, out, dtype, diag)
        ws = self._workspace("_mpc_policy_ws", L.lib().emei_mpc_policy_workspace_bytes, K)
        L.check(L.lib().emei_mpc_policy(self._h, T, H, K, C.byref(ps), C.byref(ns), _seed64(stride),
                                        L.MPC_POLICY_ACT_MEAN if act == "mean" else L.MPC_POLICY_ACT_BEST, discount,
                                        1.0 if temperature is None else temperature, _ptr(ws), _ptr(actions), _ACT_DTYPES[dtype],
                                        _ptr(obs), _ptr(rew), _ptr(done), _ptr(pr), _ptr(pi), _ptr(es),
                                        L.FLAG_AUTO_RESET if auto_reset else 0, _stream()))
        return (actions, obs, rew, done) + ((pr, pi) + ((es,) if es is not None else ()) if diagnostics else ())

    def _check_plan_out(self, name, out, shape, source, source_name):
        """an output tensor of plan_mppi / plan_cem: float32 [H, N(, act_dim)], `source` itself (in place) or clear of it"""
        if not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32 or not out.is_contiguous() \
                or not (tuple(out.shape) == shape or (self.act_dim == 1 and tuple(out.shape) == shape + (1,))):
            raise ValueError(f"{name} must be a contiguous float32 tensor {shape} on {self.device}")
        if source is not None and out.data_ptr() != source.data_ptr():
            lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * 4
            if lo < source.data_ptr() + source.numel() * 4 and source.data_ptr() < hi:
                raise ValueError(f"{name} may be {source_name} itself, not a tensor that overlaps it partly")

    @_on_device
    def plan_cem(self, H, K, n_elites, seed, discount=1.0, nominal=None, sigma=None, start_state=None, out=None, out_sigma=None,
                 elite_return=False, value=None):
        """One cross-entropy-method iteration in two launches (emei_plan_cem): the K candidates per env that plan_shooting(H, K, seed,
        nominal=, sigma=) scores are scored the same way, the n_elites best per env — the planner's order: higher return first, NaN
        last, ties to the lower index — are selected on the device, redrawn and their mean and population standard deviation taken.
        sigma: a float, or a float32 tensor of nominal's shape (one sigma per entry: the std of the previous iteration).
        -> (mean float32 [H, N(, act_dim)], std (the same shape; None for the discrete envs, whose mean is a Bernoulli probability),
        best_return float64 [N], best_index int32 [N][, elite_return float64 [N]: the return of the last candidate admitted]).
        out / out_sigma: float32 tensors to write mean / std into; they may be `nominal` / the sigma tensor themselves (in place).
        The handle is left as it is.  Other arguments as sample_candidates.
        value= (a policy.DeepValueFunction): CEM with a terminal value (emei_plan_cem_value) — the elite set, the moments, the winner
        and elite_return use the returns evaluate_sequences(..., value=) gives."""
        vs = self._plan_value(value, "plan_cem")
        sigma_map = None
        if isinstance(sigma, torch.Tensor):
            H, K, nominal, _, _ = self._candidate_args(H, K, nominal, 1.0, None)
            sigma_map, sigma = self._sigma_map(nominal, sigma), 0.0
        else:
            H, K, nominal, sigma, _ = self._candidate_args(H, K, nominal, sigma, None)
        n_elites = int(n_elites)
        if not 1 <= n_elites <= K:
            raise ValueError(f"n_elites={n_elites} is outside [1, n_candidates={K}]")
        st = self._start_rows(start_state)
        shape = (H, self.n_envs) + self._act_tail
        like = shape if nominal is None else tuple(nominal.shape)
        if out is None:
            out = torch.empty(like, dtype=torch.float32, device=self.device)
        else:
            self._check_plan_out("out", out, shape, nominal, "nominal")
        if self.act_dim == 0:
            if out_sigma is not None:
                raise ValueError("a discrete env has no standard deviation: out_sigma must be None")
        elif out_sigma is None:
            out_sigma = torch.empty(like, dtype=torch.float32, device=self.device)
        else:
            self._check_plan_out("out_sigma", out_sigma, shape, sigma_map, "the sigma tensor")
        if vs is None:
            ws = self._workspace("_cem_ws", L.lib().emei_plan_cem_workspace_bytes, K)
        else:
            ws = self._workspace("_plan_value_ws", L.lib().emei_plan_value_workspace_bytes, K)
        ret = torch.empty(self.n_envs, dtype=torch.float64, device=self.device)
        idx = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        er = torch.empty(self.n_envs, dtype=torch.float64, device=self.device) if elite_return else None
        head = (self._h, H, K, n_elites, _seed64(seed), _ptr(nominal), sigma, _ptr(sigma_map), float(discount))
        tail = (_ptr(st), _ptr(ws), _ptr(out), _ptr(out_sigma), _ptr(ret), _ptr(idx), _ptr(er), _stream())
        if vs is None:
            L.check(L.lib().emei_plan_cem(*head, *tail))
        else:
            L.check(L.lib().emei_plan_cem_value(*head, C.byref(vs), *tail))
        return (out, out_sigma, ret, idx) + ((er,) if elite_return else ())

    @_on_device
    def capture_step_graph(self, actions, auto_reset=False):
        """Capture one emei_step launch per row of `actions` [K, N(,act_dim)] into a hipGraph.

        For callers that need a launch per env-step (e.g. a policy evaluated between steps is captured
        alongside) the graph removes the per-launch host cost (6.7 -> 3.7 us per step at 65 536 envs).
        The ABI's launch functions neither allocate nor synchronise, so they are capturable as they
        are.  Returns (graph, obs [K,N,obs_dim], reward [K,N], done [K,N]); `actions` and the outputs are
        the graph's static buffers: refill `actions` in place, then `graph.replay()`."""
        K = int(actions.shape[0])
        dt = self._check_actions(actions, (K,))
        obs, rew, done = self.alloc_outputs(K)
        flags = L.FLAG_AUTO_RESET if auto_reset else 0
        lib = L.lib()

        def launch_all():
            st = _stream()
            for k in range(K):
                L.check(lib.emei_step(self._h, _ptr(actions[k]), dt, _ptr(obs[k]), _ptr(rew[k]), _ptr(done[k]), flags, st))

        if not self.get_state().isfinite().any():  # touches the state: also asserts reset() happened
            raise L.EmeiHipError("capture_step_graph: state has no finite entry")
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            launch_all()
        torch.cuda.current_stream().wait_stream(side)
        return graph, obs, rew, done

    def alloc_outputs(self, n_steps=None):
        lead = () if n_steps is None else (int(n_steps),)
        return (torch.empty(lead + (self.n_envs, self.obs_dim), dtype=torch.float32, device=self.device),
                torch.empty(lead + (self.n_envs,), dtype=torch.float32, device=self.device),
                torch.empty(lead + (self.n_envs,), dtype=torch.uint8, device=self.device))

    @_on_device
    def get_counters(self):
        """(steps since reset int32 [N], episode index int64 [N])."""
        steps = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        epi = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)  # uint32 payload
        L.check(L.lib().emei_get_counters(self._h, _ptr(steps), _ptr(epi), _stream()))
        return steps, epi.to(torch.int64) & 0xFFFFFFFF

    @_on_device
    def episode_init_obs(self, env_index, episode):
        """Initial observation of the device reset for (env, episode) pairs -> [count, obs_dim] float32."""
        env_index = env_index.to(device=self.device, dtype=torch.int64).contiguous()
        epi = (episode.to(device=self.device, dtype=torch.int64) & 0xFFFFFFFF).to(torch.int32).contiguous()  # uint32 payload
        out = torch.empty((env_index.numel(), self.obs_dim), dtype=torch.float32, device=self.device)
        if env_index.numel():
            L.check(L.lib().emei_episode_init_obs(self._h, env_index.numel(), _ptr(env_index), _ptr(epi), _ptr(out), _stream()))
        return out

    @_on_device
    def compact_done(self):
        """Sorted indices of the envs that were done at the last step (int32 tensor)."""
        idx = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
        L.check(L.lib().emei_compact_done(self._h, _ptr(idx), _ptr(cnt), _stream()))
        return idx[: int(cnt.item())]


# -- stateless batched functions -----------------------------------------------------------------
def _rows(t, device, dtype=None):
    """caller's array -> contiguous device tensor; float64 stays float64 (the reference evaluates these functions on float64
    arrays: cartpole.py:124-129,145-151; half_cheetah.py:59-67), anything else becomes float32"""
    if t is None:
        return None
    t = torch.as_tensor(t, device=device)
    if dtype is None:
        dtype = torch.float64 if t.dtype == torch.float64 else torch.float32
    return t.to(dtype).contiguous()


def _io(t):
    return L.IO_F64 if t.dtype == torch.float64 else L.IO_F32


def batch_reward(env_name, obs, pre_obs=None, action=None, real_time_scale=0.02, freq_rate=1, env_params=None,
                 batch_ctrl_cost=False):
    """get_batch_reward on [B, obs_dim] rows -> [B] in the rows' dtype (float64 in -> float64 out, not narrowed).
    batch_ctrl_cost: HalfCheetah / Hopper only — the control cost summed over the WHOLE batch, which is what
    half_cheetah.py:61 / hopper.py:98 execute for B > 1 (np.sum without an axis)."""
    obs = _rows(obs, obs.device if isinstance(obs, torch.Tensor) else "cuda")
    pre_obs, action = _rows(pre_obs, obs.device, obs.dtype), _rows(action, obs.device, obs.dtype)
    out = torch.empty(obs.shape[0], dtype=obs.dtype, device=obs.device)
    mask, arr = L.pack_env_params(env_params)
    with torch.cuda.device(obs.device):
        L.check(L.lib().emei_reward_io(L.ENV_IDS[env_name], obs.shape[0], _io(obs), _ptr(obs), _ptr(pre_obs), _ptr(action),
                                       float(real_time_scale), int(freq_rate), mask, C.cast(arr, C.c_void_p),
                                       L.REWARD_BATCH_CTRL_COST if batch_ctrl_cost else 0, _ptr(out), _stream()))
    return out


def batch_terminal(env_name, obs, env_params=None):
    obs = _rows(obs, obs.device if isinstance(obs, torch.Tensor) else "cuda")
    out = torch.empty(obs.shape[0], dtype=torch.uint8, device=obs.device)
    mask, arr = L.pack_env_params(env_params)
    with torch.cuda.device(obs.device):
        L.check(L.lib().emei_terminal_io(L.ENV_IDS[env_name], obs.shape[0], _io(obs), _ptr(obs), mask, C.cast(arr, C.c_void_p),
                                         _ptr(out), _stream()))
    return out.bool()


def batch_next_obs(env_name, obs, actions, real_time_scale=0.02, freq_rate=1, precision="ref", integrator="euler", ode_method="euler"):
    """ode_method: classic control only (ODE_approximation's `method`, base_control.py:133-173)"""
    obs = _rows(obs, obs.device if isinstance(obs, torch.Tensor) else "cuda")
    actions = actions.to(obs.device).contiguous()
    out = torch.empty_like(obs)
    with torch.cuda.device(obs.device):
        L.check(L.lib().emei_next_obs_io(L.ENV_IDS[env_name], obs.shape[0], _io(obs), _ptr(obs), _ptr(actions),
                                         _ACT_DTYPES[actions.dtype], float(real_time_scale), int(freq_rate),
                                         {"ref": 0, "f32": 1}[precision],
                                         L.INTEGRATORS[integrator] | (L.NEXT_OBS_ODE_RK4 if L.ODE_METHODS[ode_method] else 0), _ptr(out), _stream()))
    return out
