"""Feedback policies the engine evaluates INSIDE a rollout launch (emei_rollout_policy, include/emei_hip.h).

MLPPolicy holds the weights of a small network — one ReLU hidden layer, or affine — as contiguous float32 device tensors;
DeepMLPPolicy, its subclass, a network with two ReLU hidden layers (emei_rollout_policy_deep: the shape of the zoo's SAC / TD3 actors).
Engine.rollout_policy hands their pointers to the kernel (with noise=PolicyNoise: emei_rollout_policy_noisy, exploration noise drawn
inside the kernel); calling the object, `policy(obs)`, evaluates the same normative
arithmetic (float64 sums in ascending index order) with torch operations, so the one object also serves the per-step path
(`datasets.collect(env, n, policy=lambda o: policy(o))`) and gives the same actions there.
DeepValueFunction holds a two-hidden-layer network with one output, the terminal value of Engine.plan_policy(..., value=)
(emei_plan_policy_deep).
"""
import ctypes as C

import torch

from . import _lib as L
from .engine import _CTRL_RANGE

_OUT_MODES = {"clip": L.POLICY_OUT_CLIP, "tanh": L.POLICY_OUT_TANH}


class MLPPolicy:
    """a = pi(obs): h = relu(w1 @ obs + b1) (or h = obs without a hidden layer), y = w2 @ h + b2, then
    out="clip": a = clip(float32(y), lo, hi);  out="tanh": a = mid + half * tanh(y) onto [lo, hi], the env's ctrlrange;
    discrete envs (one output): a = 1 if y >= 0 else 0, whatever `out` says.
    w2 [n_out, hidden] (or [n_out, obs_dim] without a hidden layer), b2 [n_out], w1 [hidden, obs_dim], b1 [hidden]: anything
    torch.as_tensor takes; kept as contiguous float32 tensors and moved to the engine's device on first use there."""

    def __init__(self, w2, b2, w1=None, b1=None, out="clip"):
        if out not in _OUT_MODES:
            raise ValueError(f"out {out!r}: 'clip' or 'tanh'")
        if (w1 is None) != (b1 is None):
            raise ValueError("w1 and b1 come together (both None: an affine policy)")
        f = lambda t: None if t is None else torch.as_tensor(t).detach().to(torch.float32).contiguous()
        self.w1, self.b1, self.w2, self.b2 = f(w1), f(b1), f(w2), f(b2)
        self.out = out
        if self.w2.dim() != 2 or self.b2.dim() != 1 or self.b2.shape[0] != self.w2.shape[0]:
            raise ValueError(f"w2 {tuple(self.w2.shape)} must be [n_out, n_in] and b2 {tuple(self.b2.shape)} [n_out]")
        self.hidden = 0
        if self.w1 is not None:
            if self.w1.dim() != 2 or self.b1.dim() != 1 or self.b1.shape[0] != self.w1.shape[0] or self.w2.shape[1] != self.w1.shape[0]:
                raise ValueError(f"w1 {tuple(self.w1.shape)} must be [hidden, obs_dim], b1 {tuple(self.b1.shape)} [hidden] and "
                                 f"w2 {tuple(self.w2.shape)} [n_out, hidden]")
            self.hidden = int(self.w1.shape[0])
            if not 1 <= self.hidden <= L.POLICY_MAX_HIDDEN:
                raise ValueError(f"hidden={self.hidden} is outside [1, {L.POLICY_MAX_HIDDEN}]")
        self.obs_dim = int(self.w1.shape[1] if self.w1 is not None else self.w2.shape[1])
        self.n_out = int(self.w2.shape[0])
        self.lo = self.hi = None  # the ctrlrange of the env the policy was last bound to (what __call__ maps onto)
        self.discrete = None

    @classmethod
    def from_module(cls, seq):
        """torch.nn.Sequential(Linear[, ReLU, Linear[, ReLU, Linear]][, Tanh]) -> MLPPolicy (a DeepMLPPolicy for two hidden layers);
        a trailing Tanh selects out="tanh"."""
        mods = list(seq)
        out = "clip"
        if mods and isinstance(mods[-1], torch.nn.Tanh):
            out, mods = "tanh", mods[:-1]
        kinds = [type(m) for m in mods]
        lin, relu = torch.nn.Linear, torch.nn.ReLU
        if kinds == [lin]:
            first, last = None, mods[0]
        elif kinds == [lin, relu, lin]:
            first, last = mods[0], mods[2]
        elif kinds == [lin, relu, lin, relu, lin]:
            if any(m.bias is None for m in mods[::2]):
                raise ValueError("from_module: every Linear needs a bias")
            return DeepMLPPolicy(mods[4].weight, mods[4].bias, mods[2].weight, mods[2].bias, mods[0].weight, mods[0].bias, out=out)
        else:
            raise ValueError("from_module takes Linear[, ReLU, Linear[, ReLU, Linear]][, Tanh]; got "
                             + ", ".join(k.__name__ for k in map(type, seq)))
        for m in (first, last):
            if m is not None and m.bias is None:
                raise ValueError("from_module: every Linear needs a bias")
        return cls(last.weight, last.bias, None if first is None else first.weight, None if first is None else first.bias, out=out)

    def to(self, device):
        for k in ("w1", "b1", "w2", "b2"):
            t = getattr(self, k)
            if t is not None and t.device != torch.device(device):
                setattr(self, k, t.to(device).contiguous())
        return self

    def bind(self, engine):
        """check the shapes against `engine`'s env, move the weights to its device, remember its ctrlrange"""
        n_out = engine.act_dim if engine.act_dim > 0 else 1
        if self.obs_dim != engine.obs_dim or self.n_out != n_out:
            raise ValueError(f"policy maps {self.obs_dim} -> {self.n_out} but {engine.env_name} has obs_dim={engine.obs_dim} and "
                             f"{n_out} policy output(s)")
        self.to(engine.device)
        self.discrete = engine.act_dim == 0
        self.lo, self.hi = _CTRL_RANGE.get(engine.env_name, (-1.0, 1.0))  # the ctrlrange of the kernels' model constants
        return self

    def struct(self):
        """struct emei_policy over the weights (which the caller keeps alive for the launch)"""
        p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        return L.EmeiPolicy(C.sizeof(L.EmeiPolicy), self.hidden, _OUT_MODES[self.out], 0, p(self.w1), p(self.b1), p(self.w2), p(self.b2))

    def __call__(self, obs, noise=None, t=None, candidate=0):
        """obs [N, obs_dim] -> actions [N] int64 (discrete), [N] float32 (one control) or [N, act_dim] float32: the normative
        arithmetic of emei_rollout_policy in torch float64 (products of float32 values are exact there; the sums run in ascending
        index order, one elementwise operation per term).  Needs bind(engine) first (Engine.rollout_policy does it).
        noise, t: a bound PolicyNoise and the step index — the action step t of emei_rollout_policy_noisy takes on these rows
        (row n is env n of the engine `noise` is bound to), the exploration term from noise.draws(engine, t): the same actions as the launch,
        bit for bit under out="clip" with a given std and on the discrete envs.
        candidate: whose word stream the exploration term is drawn from — k > 0: the action candidate k of Engine.plan_policy takes at
        step t on these rows (its candidate 0 takes no noise at all: policy(obs)); the default 0 is the rollout's own stream."""
        if self.discrete is None:
            raise ValueError("MLPPolicy: bind(engine) first (which env's action space is this for?)")
        if (noise is None) != (t is None):
            raise ValueError("noise and t come together")
        x = torch.as_tensor(obs, device=self.w2.device).to(torch.float32).to(torch.float64)
        if self.hidden:
            z = self.b1.to(torch.float64)[None, :].repeat(x.shape[0], 1)
            w1 = self.w1.to(torch.float64)
            for k in range(self.obs_dim):
                z = z + w1[None, :, k] * x[:, k:k + 1]
            h = z.to(torch.float32)
            h = torch.where(h > 0, h, torch.zeros_like(h)).to(torch.float64)
        else:
            h = x
        y = self.b2.to(torch.float64)[None, :].repeat(x.shape[0], 1)
        w2 = self.w2.to(torch.float64)
        for j in range(h.shape[1]):
            y = y + w2[None, :, j] * h[:, j:j + 1]
        return self._output(x, h, y, noise, t, candidate)

    def _output(self, x, h, y, noise, t, candidate=0):
        """what follows y: the threshold / epsilon-greedy of the discrete envs, or the noise term and the clip / tanh clause; h is what
        the output layer read (the log-std head reads it too)"""
        if self.discrete:
            greedy = (y[:, 0] >= 0).to(torch.int64)
            if noise is None:
                return greedy
            explore, coin = noise.draws(noise.bound_engine(), t, candidate)
            return torch.where(explore != 0, coin.to(torch.int64), greedy)
        if noise is not None:  # the last term of the sum: y_q + (double)s_q * (double)z_q
            z = noise.draws(noise.bound_engine(), t, candidate).reshape(x.shape[0], self.n_out)
            y = y + noise.scale(h).to(torch.float64) * z.to(torch.float64)
        if self.out == "tanh":
            a = (0.5 * (self.hi + self.lo) + 0.5 * (self.hi - self.lo) * torch.tanh(y)).to(torch.float32)
        else:
            a = y.to(torch.float32)
            a = torch.where(a >= self.lo, a, torch.full_like(a, self.lo))  # fmaxf(a, lo): NaN -> lo
            a = torch.where(a <= self.hi, a, torch.full_like(a, self.hi))
        return a[:, 0].contiguous() if self.n_out == 1 else a.contiguous()


class DeepMLPPolicy(MLPPolicy):
    """a = pi(obs) with TWO ReLU hidden layers: h1 = relu(w1 @ obs + b1), h2 = relu(w2 @ h1 + b2), y = w3 @ h2 + b3, then MLPPolicy's
    output clause (clip / tanh / threshold).  w3 [n_out, hidden2], b3 [n_out], w2 [hidden2, hidden1], b2 [hidden2],
    w1 [hidden1, obs_dim], b1 [hidden1], both widths in 1 .. 256 (emei_rollout_policy_deep, include/emei_hip.h).  An MLPPolicy
    wherever one is taken: Engine.rollout_policy (noise= included; a log_std_head reads h2: ws [n_out, hidden2]),
    Engine.evaluate_policies, datasets.collect; calling it evaluates the same normative arithmetic in torch float64."""

    _WEIGHTS = ("w1", "b1", "w2", "b2", "w3", "b3")

    def __init__(self, w3, b3, w2, b2, w1, b1, out="clip"):
        if out not in _OUT_MODES:
            raise ValueError(f"out {out!r}: 'clip' or 'tanh'")
        f = lambda t: torch.as_tensor(t).detach().to(torch.float32).contiguous()
        self.w1, self.b1, self.w2, self.b2, self.w3, self.b3 = f(w1), f(b1), f(w2), f(b2), f(w3), f(b3)
        self.out = out
        for w, b, name in ((self.w1, self.b1, "1"), (self.w2, self.b2, "2"), (self.w3, self.b3, "3")):
            if w.dim() != 2 or b.dim() != 1 or b.shape[0] != w.shape[0]:
                raise ValueError(f"w{name} {tuple(w.shape)} must be [n, n_in] and b{name} {tuple(b.shape)} [n]")
        if self.w2.shape[1] != self.w1.shape[0]:
            raise ValueError(f"w2 {tuple(self.w2.shape)} must be [hidden2, hidden1] with hidden1 = {int(self.w1.shape[0])} (w1's rows)")
        if self.w3.shape[1] != self.w2.shape[0]:
            raise ValueError(f"w3 {tuple(self.w3.shape)} must be [n_out, hidden2] with hidden2 = {int(self.w2.shape[0])} (w2's rows)")
        self.hidden1, self.hidden2 = int(self.w1.shape[0]), int(self.w2.shape[0])
        for name, v in (("hidden1", self.hidden1), ("hidden2", self.hidden2)):
            if not 1 <= v <= L.POLICY_DEEP_MAX_HIDDEN:
                raise ValueError(f"{name}={v} is outside [1, {L.POLICY_DEEP_MAX_HIDDEN}]")
        self.hidden = self.hidden2  # the width the output layer (and a log-std head) reads
        self.obs_dim = int(self.w1.shape[1])
        self.n_out = int(self.w3.shape[0])
        self.lo = self.hi = None
        self.discrete = None

    def to(self, device):
        for k in self._WEIGHTS:
            t = getattr(self, k)
            if t.device != torch.device(device):
                setattr(self, k, t.to(device).contiguous())
        return self

    def struct(self):
        """struct emei_policy_deep over the weights (which the caller keeps alive for the launch)"""
        p = lambda t: C.c_void_p(t.data_ptr())
        return L.EmeiPolicyDeep(C.sizeof(L.EmeiPolicyDeep), self.hidden1, self.hidden2, _OUT_MODES[self.out], p(self.w1), p(self.b1),
                                p(self.w2), p(self.b2), p(self.w3), p(self.b3), 0)

    def __call__(self, obs, noise=None, t=None, candidate=0):
        """MLPPolicy.__call__ for the two-hidden-layer network: the normative arithmetic of emei_rollout_policy_deep in torch float64,
        one elementwise operation per term, every sum in ascending index order; the same actions as the launch (bit for bit where
        MLPPolicy's are)."""
        if self.discrete is None:
            raise ValueError("DeepMLPPolicy: bind(engine) first (which env's action space is this for?)")
        if (noise is None) != (t is None):
            raise ValueError("noise and t come together")
        h = torch.as_tensor(obs, device=self.w3.device).to(torch.float32).to(torch.float64)
        x = h
        for w, b in ((self.w1, self.b1), (self.w2, self.b2)):
            z = b.to(torch.float64)[None, :].repeat(h.shape[0], 1)
            w = w.to(torch.float64)
            for k in range(h.shape[1]):
                z = z + w[None, :, k] * h[:, k:k + 1]
            h = z.to(torch.float32)
            h = torch.where(h > 0, h, torch.zeros_like(h)).to(torch.float64)
        y = self.b3.to(torch.float64)[None, :].repeat(h.shape[0], 1)
        w3 = self.w3.to(torch.float64)
        for i in range(h.shape[1]):
            y = y + w3[None, :, i] * h[:, i:i + 1]
        return self._output(x, h, y, noise, t, candidate)


class DeepValueFunction:
    """V(obs) with TWO ReLU hidden layers and one output: the terminal value of Engine.plan_policy(..., value=)
    (emei_plan_policy_deep, include/emei_hip.h) — h1 = relu(w1 @ obs + b1), h2 = relu(w2 @ h1 + b2), v = float32(w3 @ h2 + b3), with
    no output clause.  w3 [1, hidden2], b3 [1], w2 [hidden2, hidden1], b2 [hidden2], w1 [hidden1, obs_dim], b1 [hidden1]; the widths
    are its own, each in 1 .. 256.  Kept as contiguous float32 tensors; calling it evaluates the normative arithmetic in torch
    float64."""

    _WEIGHTS = DeepMLPPolicy._WEIGHTS

    def __init__(self, w3, b3, w2, b2, w1, b1):
        f = lambda t: torch.as_tensor(t).detach().to(torch.float32).contiguous()
        self.w1, self.b1, self.w2, self.b2, self.w3, self.b3 = f(w1), f(b1), f(w2), f(b2), f(w3), f(b3)
        for w, b, name in ((self.w1, self.b1, "1"), (self.w2, self.b2, "2"), (self.w3, self.b3, "3")):
            if w.dim() != 2 or b.dim() != 1 or b.shape[0] != w.shape[0]:
                raise ValueError(f"w{name} {tuple(w.shape)} must be [n, n_in] and b{name} {tuple(b.shape)} [n]")
        if self.w2.shape[1] != self.w1.shape[0]:
            raise ValueError(f"w2 {tuple(self.w2.shape)} must be [hidden2, hidden1] with hidden1 = {int(self.w1.shape[0])} (w1's rows)")
        if self.w3.shape[1] != self.w2.shape[0]:
            raise ValueError(f"w3 {tuple(self.w3.shape)} must be [1, hidden2] with hidden2 = {int(self.w2.shape[0])} (w2's rows)")
        if self.w3.shape[0] != 1:
            raise ValueError(f"w3 {tuple(self.w3.shape)} must be [1, hidden2]: a value function has one output")
        self.hidden1, self.hidden2 = int(self.w1.shape[0]), int(self.w2.shape[0])
        for name, v in (("hidden1", self.hidden1), ("hidden2", self.hidden2)):
            if not 1 <= v <= L.POLICY_DEEP_MAX_HIDDEN:
                raise ValueError(f"{name}={v} is outside [1, {L.POLICY_DEEP_MAX_HIDDEN}]")
        self.obs_dim = int(self.w1.shape[1])

    @classmethod
    def from_module(cls, seq):
        """torch.nn.Sequential(Linear, ReLU, Linear, ReLU, Linear(hidden2, 1)) -> DeepValueFunction, as MLPPolicy.from_module reads an
        actor; a value has no output clause, so nothing may follow the last Linear."""
        mods = list(seq)
        lin, relu = torch.nn.Linear, torch.nn.ReLU
        if [type(m) for m in mods] != [lin, relu, lin, relu, lin]:
            raise ValueError("DeepValueFunction.from_module takes Linear, ReLU, Linear, ReLU, Linear(hidden2, 1); got "
                             + ", ".join(type(m).__name__ for m in mods))
        if any(m.bias is None for m in mods[::2]):
            raise ValueError("from_module: every Linear needs a bias")
        return cls(mods[4].weight, mods[4].bias, mods[2].weight, mods[2].bias, mods[0].weight, mods[0].bias)

    to = DeepMLPPolicy.to  # to(device): the weights moved in place, returns self

    def bind(self, engine):
        """check obs_dim against `engine`'s env and move the weights to its device"""
        if self.obs_dim != engine.obs_dim:
            raise ValueError(f"value function reads {self.obs_dim} inputs but {engine.env_name} has obs_dim={engine.obs_dim}")
        return self.to(engine.device)

    def struct(self):
        """struct emei_policy_deep over the weights (which the caller keeps alive for the launch); out_mode is ignored for a value"""
        p = lambda t: C.c_void_p(t.data_ptr())
        return L.EmeiPolicyDeep(C.sizeof(L.EmeiPolicyDeep), self.hidden1, self.hidden2, L.POLICY_OUT_CLIP, p(self.w1), p(self.b1),
                                p(self.w2), p(self.b2), p(self.w3), p(self.b3), 0)

    def __call__(self, obs):
        """obs [N, obs_dim] -> v float32 [N]: the value clause of emei_plan_policy_deep in torch float64, one elementwise operation
        per term, every sum in ascending index order; v = float32(y_0) with no output clause (a NaN stays a NaN)."""
        h = torch.as_tensor(obs, device=self.w3.device).to(torch.float32).to(torch.float64)
        for w, b in ((self.w1, self.b1), (self.w2, self.b2)):
            z = b.to(torch.float64)[None, :].repeat(h.shape[0], 1)
            w = w.to(torch.float64)
            for k in range(h.shape[1]):
                z = z + w[None, :, k] * h[:, k:k + 1]
            h = z.to(torch.float32)
            h = torch.where(h > 0, h, torch.zeros_like(h)).to(torch.float64)
        y = self.b3.to(torch.float64)[None, :].repeat(h.shape[0], 1)
        w3 = self.w3.to(torch.float64)
        for i in range(h.shape[1]):
            y = y + w3[None, :, i] * h[:, i:i + 1]
        return y[:, 0].to(torch.float32).contiguous()


class PolicyNoise:
    """The exploration noise of Engine.rollout_policy(..., noise=) (emei_rollout_policy_noisy, include/emei_hip.h), drawn inside the
    kernel from the word stream of (seed + t, global env index).  Exactly one of
      std: a float or [n_out] values — Gaussian noise std * z on the continuous envs, added to the network's output before clip / tanh;
      log_std_head=(ws [n_out, hidden] (or [n_out, obs_dim] without a hidden layer), bs [n_out]): the std is exp(clamp(ws @ h + bs,
          *log_std_range)), a second head on the policy's hidden layer (SAC's actor with out="tanh");
      epsilon: in [0, 1] — epsilon-greedy on the discrete envs: with probability epsilon a fair coin replaces the policy's action."""

    def __init__(self, seed, std=None, epsilon=None, log_std_head=None, log_std_range=(-20.0, 2.0)):
        if sum(v is not None for v in (std, epsilon, log_std_head)) != 1:
            raise ValueError("PolicyNoise takes exactly one of std=, epsilon= and log_std_head=")
        self.seed = int(seed)
        self.sigma, self.std, self.ws, self.bs = 0.0, None, None, None
        self.log_std_min, self.log_std_max = (float(v) for v in log_std_range)
        f = lambda v: torch.as_tensor(v).detach().to(torch.float32).contiguous()
        if epsilon is not None:
            self.mode, self.sigma = L.POLICY_NOISE_EPS_GREEDY, float(epsilon)
            if not 0.0 <= self.sigma <= 1.0:
                raise ValueError(f"epsilon={epsilon} is outside [0, 1]")
        elif log_std_head is not None:
            self.mode = L.POLICY_NOISE_GAUSS_HEAD
            self.ws, self.bs = (f(v) for v in log_std_head)
            if self.ws.dim() != 2 or self.bs.dim() != 1 or self.bs.shape[0] != self.ws.shape[0]:
                raise ValueError(f"log_std_head: ws {tuple(self.ws.shape)} must be [n_out, n_in] and bs {tuple(self.bs.shape)} [n_out]")
            if not self.log_std_min <= self.log_std_max:
                raise ValueError(f"log_std_range={log_std_range}: min <= max, neither NaN")
        else:
            self.mode = L.POLICY_NOISE_GAUSS
            if torch.as_tensor(std).dim() == 0:
                self.sigma = float(std)
                if not (self.sigma >= 0.0 and self.sigma != float("inf")):
                    raise ValueError(f"std={std} must be finite and >= 0")
            else:
                self.std = f(std)
                if self.std.dim() != 1:
                    raise ValueError(f"std {tuple(self.std.shape)} must be a float or [n_out] values")
        self._engine = None

    def bind(self, engine):
        """check the mode against `engine`'s env kind and the shapes against its action space; move the tensors to its device"""
        discrete = engine.act_dim == 0
        if discrete != (self.mode == L.POLICY_NOISE_EPS_GREEDY):
            raise ValueError(f"{engine.env_name} is a {'discrete' if discrete else 'continuous'} env: epsilon= is for the discrete envs, "
                             "std= and log_std_head= for the continuous ones")
        n_out = engine.act_dim if engine.act_dim > 0 else 1
        for k in ("std", "ws", "bs"):
            v = getattr(self, k)
            if v is not None:
                if v.shape[0] != n_out:
                    raise ValueError(f"noise {k} {tuple(v.shape)}: {engine.env_name} has {n_out} policy output(s)")
                setattr(self, k, v.to(engine.device).contiguous())
        self._engine = engine
        return self

    def bound_engine(self):
        if self._engine is None:
            raise ValueError("PolicyNoise: bind(engine) first")
        return self._engine

    def struct(self, hidden_in=None):
        """struct emei_policy_noise over the tensors (which the caller keeps alive for the launch); hidden_in: the width the policy's
        output layer reads, which the log-std head must read too"""
        if self.ws is not None and hidden_in is not None and self.ws.shape[1] != hidden_in:
            raise ValueError(f"log_std_head: ws {tuple(self.ws.shape)} must be [n_out, {hidden_in}] like the policy's w2")
        p = lambda v: C.c_void_p(0 if v is None else v.data_ptr())
        return L.EmeiPolicyNoise(C.sizeof(L.EmeiPolicyNoise), self.mode, self.seed & (2**64 - 1), self.sigma, p(self.std), p(self.ws),
                                 p(self.bs), self.log_std_min, self.log_std_max, 0)

    def draws(self, engine, t, candidate=0):
        """what step t draws for every env of `engine`, obtained from the DEVICE through Engine.sample_candidates (candidate 0
        under the key seed + t is the noise stream; candidate k > 0 is the stream of Engine.plan_policy's candidate k).  Continuous envs: z float32 [N(, act_dim)] = 8 * (the clipped Gaussian candidate
        with mean 0 and sigma 0.125) — exact: |z| <= 5.77, so 0.125 z never reaches a ctrlrange of +-1 or +-3, and scaling by a power
        of two is exact.  Discrete envs: (explore, coin) [N] int64, the Bernoulli draws with p = epsilon at t = 0 and p = 0.5 at t = 1."""
        eng = engine
        key = self.seed + int(t)
        k = int(candidate)
        if k < 0:
            raise ValueError(f"candidate={candidate} must be >= 0")
        if eng.act_dim == 0:
            nominal = torch.tensor([self.sigma, 0.5], dtype=torch.float32, device=eng.device)[:, None].repeat(1, eng.n_envs).contiguous()
            d = eng.sample_candidates(2, k + 1, key, nominal=nominal)
            return d[0, :, k], d[1, :, k]
        zeros = torch.zeros((1, eng.n_envs) + eng._act_tail, dtype=torch.float32, device=eng.device)
        return 8.0 * eng.sample_candidates(1, k + 1, key, nominal=zeros, sigma=0.125)[0, :, k]

    def scale(self, h):
        """s [N, n_out] float32 for the rows whose hidden activations (float64 [N, hidden], or the inputs without a hidden layer)
        are h: the given std, or the log-std head's float32(exp(clamp(l)))"""
        if self.mode == L.POLICY_NOISE_GAUSS:
            s = self.std if self.std is not None else torch.full((1,), self.sigma, dtype=torch.float32, device=h.device)
            return s[None, :].expand(h.shape[0], -1)
        lq = self.bs.to(torch.float64)[None, :].repeat(h.shape[0], 1)
        ws = self.ws.to(torch.float64)
        for j in range(h.shape[1]):
            lq = lq + ws[None, :, j] * h[:, j:j + 1]
        lq = torch.clamp(lq, self.log_std_min, self.log_std_max)
        return torch.exp(lq).to(torch.float32)


class PolicyPopulation:
    """P policies of one architecture stacked along a leading axis, for Engine.evaluate_policies (emei_evaluate_policies):
    w2 [P, n_out, hidden] (or [P, n_out, obs_dim] without a hidden layer), b2 [P, n_out], w1 [P, hidden, obs_dim], b1 [P, hidden];
    `out` is shared.  Kept as contiguous float32 tensors: member p's weights sit at p * (the member's size) behind each base
    pointer, which is the layout the kernels offset into.  len(pop) is P; pop[p] is an MLPPolicy viewing member p."""

    def __init__(self, w2, b2, w1=None, b1=None, out="clip"):
        if out not in _OUT_MODES:
            raise ValueError(f"out {out!r}: 'clip' or 'tanh'")
        if (w1 is None) != (b1 is None):
            raise ValueError("w1 and b1 come together (both None: affine policies)")
        f = lambda t: None if t is None else torch.as_tensor(t).detach().to(torch.float32).contiguous()
        self.w1, self.b1, self.w2, self.b2 = f(w1), f(b1), f(w2), f(b2)
        self.out = out
        if self.w2.dim() != 3 or self.w2.shape[0] < 1:
            raise ValueError(f"w2 {tuple(self.w2.shape)} must be [P, n_out, n_in] with P >= 1")
        P = int(self.w2.shape[0])
        if self.b2.dim() != 2 or tuple(self.b2.shape) != (P, self.w2.shape[1]):
            raise ValueError(f"b2 {tuple(self.b2.shape)} must be [P, n_out] = {(P, int(self.w2.shape[1]))}")
        self.hidden = 0
        if self.w1 is not None:
            if self.w1.dim() != 3 or self.w1.shape[0] != P:
                raise ValueError(f"w1 {tuple(self.w1.shape)} must be [P, hidden, obs_dim] with P = {P}")
            if tuple(self.b1.shape) != (P, self.w1.shape[1]):
                raise ValueError(f"b1 {tuple(self.b1.shape)} must be [P, hidden] = {(P, int(self.w1.shape[1]))}")
            if self.w2.shape[2] != self.w1.shape[1]:
                raise ValueError(f"w2 {tuple(self.w2.shape)} must be [P, n_out, hidden] with hidden = {int(self.w1.shape[1])}")
            self.hidden = int(self.w1.shape[1])
            if not 1 <= self.hidden <= L.POLICY_MAX_HIDDEN:
                raise ValueError(f"hidden={self.hidden} of w1 is outside [1, {L.POLICY_MAX_HIDDEN}]")
        self.n_policies = P
        self.obs_dim = int(self.w1.shape[2] if self.w1 is not None else self.w2.shape[2])
        self.n_out = int(self.w2.shape[1])
        self._engine = None

    @classmethod
    def from_policies(cls, policies):
        """[MLPPolicy, ...] of the same shapes and the same `out` -> the population holding copies of their weights"""
        policies = list(policies)
        if not policies or not all(isinstance(p, MLPPolicy) for p in policies):
            raise ValueError("from_policies takes a non-empty list of MLPPolicy")
        if any(isinstance(p, DeepMLPPolicy) for p in policies):
            raise ValueError("from_policies: a DeepMLPPolicy belongs in a DeepPolicyPopulation")
        first = policies[0]
        for n, p in enumerate(policies):
            if p.out != first.out:
                raise ValueError(f"policy {n}: out={p.out!r} differs from policy 0's {first.out!r}")
            for k in ("w1", "b1", "w2", "b2"):
                a, b = getattr(first, k), getattr(p, k)
                if (a is None) != (b is None) or (a is not None and a.shape != b.shape):
                    raise ValueError(f"policy {n}: {k} {None if b is None else tuple(b.shape)} differs from policy 0's "
                                     f"{None if a is None else tuple(a.shape)}")
        dev = first.w2.device
        st = lambda k: None if getattr(first, k) is None else torch.stack([getattr(p, k).to(dev) for p in policies])
        return cls(st("w2"), st("b2"), st("w1"), st("b1"), out=first.out)

    def __len__(self):
        return self.n_policies

    def __getitem__(self, p):
        """member p as an MLPPolicy over VIEWS of the stacked weights (bound as the population is)"""
        p = int(p)
        if not -self.n_policies <= p < self.n_policies:
            raise IndexError(f"policy {p} of a population of {self.n_policies}")
        v = lambda t: None if t is None else t[p]
        m = MLPPolicy(v(self.w2), v(self.b2), v(self.w1), v(self.b1), out=self.out)
        return m.bind(self._engine) if self._engine is not None else m

    def to(self, device):
        for k in ("w1", "b1", "w2", "b2"):
            t = getattr(self, k)
            if t is not None and t.device != torch.device(device):
                setattr(self, k, t.to(device).contiguous())
        return self

    def bind(self, engine):
        """check the shapes against `engine`'s env and move the weights to its device, as MLPPolicy.bind"""
        n_out = engine.act_dim if engine.act_dim > 0 else 1
        if self.obs_dim != engine.obs_dim or self.n_out != n_out:
            raise ValueError(f"the policies map {self.obs_dim} -> {self.n_out} but {engine.env_name} has obs_dim={engine.obs_dim} and "
                             f"{n_out} policy output(s)")
        self.to(engine.device)
        self._engine = engine
        return self

    def struct(self):
        """the stacked struct emei_policy over the weights (which the caller keeps alive for the launch)"""
        p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        return L.EmeiPolicy(C.sizeof(L.EmeiPolicy), self.hidden, _OUT_MODES[self.out], 0, p(self.w1), p(self.b1), p(self.w2), p(self.b2))


class DeepPolicyPopulation:
    """P DeepMLPPolicy networks of one architecture stacked along a leading axis, for Engine.evaluate_policies
    (emei_evaluate_policies_deep): w3 [P, n_out, hidden2], b3 [P, n_out], w2 [P, hidden2, hidden1], b2 [P, hidden2],
    w1 [P, hidden1, obs_dim], b1 [P, hidden1]; `out` is shared.  Kept as contiguous float32 tensors, member p's weights at
    p * (the member's size) behind each base pointer.  len(pop) is P; pop[p] is a DeepMLPPolicy viewing member p."""

    _WEIGHTS = DeepMLPPolicy._WEIGHTS

    def __init__(self, w3, b3, w2, b2, w1, b1, out="clip"):
        if out not in _OUT_MODES:
            raise ValueError(f"out {out!r}: 'clip' or 'tanh'")
        f = lambda t: torch.as_tensor(t).detach().to(torch.float32).contiguous()
        self.w1, self.b1, self.w2, self.b2, self.w3, self.b3 = f(w1), f(b1), f(w2), f(b2), f(w3), f(b3)
        self.out = out
        if self.w3.dim() != 3 or self.w3.shape[0] < 1:
            raise ValueError(f"w3 {tuple(self.w3.shape)} must be [P, n_out, hidden2] with P >= 1")
        P = int(self.w3.shape[0])
        for w, b, name in ((self.w1, self.b1, "1"), (self.w2, self.b2, "2"), (self.w3, self.b3, "3")):
            if w.dim() != 3 or w.shape[0] != P:
                raise ValueError(f"w{name} {tuple(w.shape)} must be [P, n, n_in] with P = {P}")
            if tuple(b.shape) != (P, w.shape[1]):
                raise ValueError(f"b{name} {tuple(b.shape)} must be [P, n] = {(P, int(w.shape[1]))}")
        if self.w2.shape[2] != self.w1.shape[1]:
            raise ValueError(f"w2 {tuple(self.w2.shape)} must be [P, hidden2, hidden1] with hidden1 = {int(self.w1.shape[1])}")
        if self.w3.shape[2] != self.w2.shape[1]:
            raise ValueError(f"w3 {tuple(self.w3.shape)} must be [P, n_out, hidden2] with hidden2 = {int(self.w2.shape[1])}")
        self.hidden1, self.hidden2 = int(self.w1.shape[1]), int(self.w2.shape[1])
        for name, v in (("hidden1", self.hidden1), ("hidden2", self.hidden2)):
            if not 1 <= v <= L.POLICY_DEEP_MAX_HIDDEN:
                raise ValueError(f"{name}={v} is outside [1, {L.POLICY_DEEP_MAX_HIDDEN}]")
        self.n_policies = P
        self.obs_dim = int(self.w1.shape[2])
        self.n_out = int(self.w3.shape[1])
        self._engine = None

    @classmethod
    def from_policies(cls, policies):
        """[DeepMLPPolicy, ...] of the same shapes and the same `out` -> the population holding copies of their weights"""
        policies = list(policies)
        if not policies or not all(isinstance(p, DeepMLPPolicy) for p in policies):
            raise ValueError("from_policies takes a non-empty list of DeepMLPPolicy")
        first = policies[0]
        for n, p in enumerate(policies):
            if p.out != first.out:
                raise ValueError(f"policy {n}: out={p.out!r} differs from policy 0's {first.out!r}")
            for k in cls._WEIGHTS:
                if getattr(first, k).shape != getattr(p, k).shape:
                    raise ValueError(f"policy {n}: {k} {tuple(getattr(p, k).shape)} differs from policy 0's {tuple(getattr(first, k).shape)}")
        dev = first.w3.device
        st = lambda k: torch.stack([getattr(p, k).to(dev) for p in policies])
        return cls(st("w3"), st("b3"), st("w2"), st("b2"), st("w1"), st("b1"), out=first.out)

    def __len__(self):
        return self.n_policies

    def __getitem__(self, p):
        """member p as a DeepMLPPolicy over VIEWS of the stacked weights (bound as the population is)"""
        p = int(p)
        if not -self.n_policies <= p < self.n_policies:
            raise IndexError(f"policy {p} of a population of {self.n_policies}")
        m = DeepMLPPolicy(self.w3[p], self.b3[p], self.w2[p], self.b2[p], self.w1[p], self.b1[p], out=self.out)
        return m.bind(self._engine) if self._engine is not None else m

    def to(self, device):
        for k in self._WEIGHTS:
            t = getattr(self, k)
            if t.device != torch.device(device):
                setattr(self, k, t.to(device).contiguous())
        return self

    def bind(self, engine):
        """check the shapes against `engine`'s env and move the weights to its device, as MLPPolicy.bind"""
        n_out = engine.act_dim if engine.act_dim > 0 else 1
        if self.obs_dim != engine.obs_dim or self.n_out != n_out:
            raise ValueError(f"the policies map {self.obs_dim} -> {self.n_out} but {engine.env_name} has obs_dim={engine.obs_dim} and "
                             f"{n_out} policy output(s)")
        self.to(engine.device)
        self._engine = engine
        return self

    def struct(self):
        """the stacked struct emei_policy_deep over the weights (which the caller keeps alive for the launch)"""
        p = lambda t: C.c_void_p(t.data_ptr())
        return L.EmeiPolicyDeep(C.sizeof(L.EmeiPolicyDeep), self.hidden1, self.hidden2, _OUT_MODES[self.out], p(self.w1), p(self.b1),
                                p(self.w2), p(self.b2), p(self.w3), p(self.b3), 0)
