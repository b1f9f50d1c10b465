#!/usr/bin/env python3
"""Planning around a feedback policy, two ways, in the same run: Engine.plan_policy (emei_plan_policy: one lane per (env, candidate),
the policy evaluated in the lane, two launches, 8 + 4 act_dim bytes written per candidate) against what the API offered before the call
existed — a SECOND engine of N x K envs holding the N states tiled K times, `rollout_policy(H, policy, noise=)` on it with its
[H, N x K] outputs, and the torch reduction of rewards and done codes to returns, the arg-max and the winner's first action.  The
tiled route is the comparator; the one call is never its own yardstick.  The two do not draw the same noise (the tiled engine keys its
streams by the env index n * K + k with candidate word 0, the call by (n, k), and its candidate 0 takes none), so only the shapes of
the results are compared here; tests/test_gpu_policy_plan.py holds the call to its per-step twin bit for bit.
Method: the horizon of a shape starts at --horizon and is doubled until one call of the fused route exceeds 12 ms (so that every timed
window is above 10 ms; a shape that reaches --max-horizon below that is marked "indicative"); then, after `--warmup` untimed runs of
each route, `--repeats` rounds; every round times ONE run of each route with device events around it (the tiled route's set_state and
host overhead are inside its window), the two routes alternating inside the round so that drift hits both alike.  Reported per shape:
the median over the rounds and the spread (min, max) of either route, and the ratio of the medians.
Shapes: CartPoleSwingUp (epsilon-greedy) and HalfCheetahRunning (Gaussian), N = 256, K = 64, hidden = 64, H = 16 to start from.
--deep H1,H2 times the two-hidden-layer call instead (emei_plan_policy_deep: a DeepMLPPolicy of those widths, one-wave blocks with the
h1 tile in dynamic LDS) against the same tiled route with the deep policy in `rollout_policy`, and, for scale, the one-layer
plan_policy at hidden = H1 in the same rounds (its horizon is the deep call's).  --value adds a terminal value network of the same
widths to the deep call; the tiled route then evaluates it as a user would, three float32 torch matmuls on the last observations, and
adds discount^H * V where no step was terminal.
One JSON line per shape, one GPU process.  Run on the GPU box:
    python tools/policy_plan_timing.py [--warmup 2] [--repeats 7] [--only INDEX] [--deep H1,H2 [--value]]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emei_amd.engine import Engine  # noqa: E402
from emei_amd.policy import DeepMLPPolicy, DeepValueFunction, MLPPolicy, PolicyNoise  # noqa: E402

CHEETAH = dict(freq_rate=4, real_time_scale=0.002, init_noise=0.1)
# (env, N, K, hidden, engine kwargs)
SHAPES = [
    ("CartPoleSwingUp", 256, 64, 64, {}),
    ("HalfCheetahRunning", 256, 64, 64, CHEETAH),
]
MIN_WINDOW_MS = 12.0


def make_policy(eng, hidden):
    """HalfCheetah: random weights.  CartPoleSwingUp ends an episode when the cart leaves the rail, and a wave of the plan kernel
    leaves with its last live lane, so a policy that loses the cart would time an empty loop: the network computes y = -(x + xdot)
    (half of the hidden units carry relu(x + xdot), half relu(-(x + xdot))), a bang-bang controller that keeps the cart near the
    centre under epsilon-greedy exploration, so that every lane of both routes runs all H steps"""
    g = torch.Generator().manual_seed(1)
    n_out = max(eng.act_dim, 1)
    r = lambda *s: torch.randn(*s, generator=g) / s[-1] ** 0.5
    if eng.act_dim == 0:
        sign = torch.cat([torch.ones(hidden // 2), -torch.ones(hidden - hidden // 2)])
        w1 = torch.zeros(hidden, eng.obs_dim)
        w1[:, 0], w1[:, 1] = sign, sign  # the observation starts with (x, xdot)
        return MLPPolicy((-sign / hidden)[None, :], torch.zeros(1), w1, torch.zeros(hidden)).bind(eng)
    return MLPPolicy(r(n_out, hidden), r(n_out), r(hidden, eng.obs_dim), r(hidden)).bind(eng)


def make_deep_policy(eng, h1, h2):
    """make_policy with two hidden layers.  CartPoleSwingUp: the same controller — h1 carries relu(+-(x + xdot)), each half of h2 the
    mean of its half of h1, the output -(mean of the positive half) + (mean of the negative half) = -(x + xdot)"""
    g = torch.Generator().manual_seed(1)
    n_out = max(eng.act_dim, 1)
    r = lambda *s: torch.randn(*s, generator=g) / s[-1] ** 0.5
    if eng.act_dim == 0:
        half = lambda n: torch.cat([torch.ones(n // 2), -torch.ones(n - n // 2)]) if n > 1 else torch.ones(1)
        s1, s2 = half(h1), half(h2)
        w1 = torch.zeros(h1, eng.obs_dim)
        w1[:, 0], w1[:, 1] = s1, s1
        same = (s2[:, None] == s1[None, :]).to(torch.float32)
        w2 = same / same.sum(dim=1, keepdim=True)
        w3 = (-s2 / (s2 == 1).sum().clamp(min=1) * (s2 == 1) - s2 / (s2 == -1).sum().clamp(min=1) * (s2 == -1))[None, :]
        return DeepMLPPolicy(w3, torch.zeros(1), w2, torch.zeros(h2), w1, torch.zeros(h1)).bind(eng)
    return DeepMLPPolicy(r(n_out, h2), r(n_out), r(h2, h1), r(h2), r(h1, eng.obs_dim), r(h1)).bind(eng)


def make_value(eng, h1, h2):
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g) / s[-1] ** 0.5
    return DeepValueFunction(r(1, h2), r(1), r(h2, h1), r(h2), r(h1, eng.obs_dim), r(h1)).bind(eng)


def make_noise(eng, seed):
    return PolicyNoise(seed, epsilon=0.2) if eng.act_dim == 0 else PolicyNoise(seed, std=0.3)


def tiled_route(big, tiled_start, policy, noise, N, K, H, discount, outs, value=None):
    """what a user of the parent commit's API writes: N x K envs, per-step outputs, then the reduction in torch"""
    big.set_state(tiled_start)
    act, obs, rew, done = big.rollout_policy(H, policy, auto_reset=False, out=outs, noise=noise)
    term = (done & 1) != 0
    length = torch.where(term.any(dim=0), term.to(torch.uint8).argmax(dim=0) + 1, H)
    counted = torch.arange(H, device=big.device)[:, None] < length[None, :]
    weights = (discount ** torch.arange(H, device=big.device, dtype=torch.float64))[:, None]
    ret = (rew.to(torch.float64) * weights * counted).sum(dim=0)
    if value is not None:  # the terminal value as a user writes it: float32 matmuls on the last observations
        h = torch.relu(obs[H - 1] @ value.w1.T + value.b1)
        h = torch.relu(h @ value.w2.T + value.b2)
        v = (h @ value.w3.T + value.b3)[:, 0]
        ret = torch.where(term.any(dim=0), ret, ret + discount ** H * v.to(torch.float64))
    ret = ret.view(N, K)
    best = ret.argmax(dim=1)
    first = act[0].view((N, K) + tuple(act.shape[2:]))
    return first[torch.arange(N, device=big.device), best], ret.max(dim=1).values, best.to(torch.int32), length.min()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--max-horizon", type=int, default=4096)
    ap.add_argument("--only", type=int, default=None, help="index of the one shape to run")
    ap.add_argument("--deep", default=None, metavar="H1,H2", help="time the two-hidden-layer call at these widths")
    ap.add_argument("--value", action="store_true", help="with --deep: a terminal value network of the same widths")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_plan_timing.py needs a GPU")
    discount = 0.99
    deep = tuple(int(v) for v in args.deep.split(",")) if args.deep else None
    if deep is not None and len(deep) != 2:
        raise SystemExit("--deep takes H1,H2")
    if args.value and deep is None:
        raise SystemExit("--value comes with --deep")
    for idx, (name, N, K, hidden, kw) in enumerate(SHAPES):
        if args.only is not None and args.only != idx:
            continue
        eng, big = Engine(name, N, **kw), Engine(name, N * K, **kw)
        eng.reset(seed=0)
        big.reset(seed=0)
        start = eng.get_state().clone()
        tiled_start = start.repeat_interleave(K, dim=0).contiguous()  # env n * K + k holds env n's state
        value = big_value = one_layer = None
        if deep is None:
            policy, big_policy = make_policy(eng, hidden), make_policy(big, hidden)
        else:
            hidden = deep[0]
            policy, big_policy = make_deep_policy(eng, *deep), make_deep_policy(big, *deep)
            one_layer = make_policy(eng, hidden)
            if args.value:
                value, big_value = make_value(eng, *deep), make_value(big, *deep)
        noise, big_noise = make_noise(eng, 7), make_noise(big, 7)
        H = args.horizon

        def timed(fn):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), out

        fused = lambda: eng.plan_policy(H, K, policy, noise, discount=discount, start_state=start, length=True, value=value)
        single = lambda: eng.plan_policy(H, K, one_layer, noise, discount=discount, start_state=start, length=True)
        timed(fused)  # code objects loaded
        while timed(fused)[0] < MIN_WINDOW_MS and 2 * H <= args.max_horizon:
            H *= 2
        outs = big.alloc_outputs(H)
        tiled = lambda: tiled_route(big, tiled_start, big_policy, big_noise, N, K, H, discount, outs, big_value)
        for _ in range(args.warmup):
            timed(fused), timed(tiled)
            if one_layer is not None:
                timed(single)
        ms = {"fused": [], "tiled": [], "one_layer": []}
        for _ in range(args.repeats):
            t, a = timed(fused)
            ms["fused"].append(t)
            t, b = timed(tiled)
            ms["tiled"].append(t)
            if one_layer is not None:
                ms["one_layer"].append(timed(single)[0])
        same_shapes = all(x.shape == y.shape and x.dtype == y.dtype for x, y in zip(a[:3], b[:3]))
        med = {k: statistics.median(v) for k, v in ms.items() if v}
        extra = {}
        if deep is not None:
            extra = {"deep": list(deep), "value": bool(args.value), "one_layer_ms": round(med["one_layer"], 4),
                     "one_layer_ms_min_max": [round(min(ms["one_layer"]), 4), round(max(ms["one_layer"]), 4)],
                     "fused_over_one_layer": round(med["fused"] / med["one_layer"], 3)}
        print(json.dumps({
            **extra,
            "env": name, "n_envs": N, "n_candidates": K, "hidden": hidden, "horizon": H, "discount": discount, "repeats": args.repeats,
            "fused_ms": round(med["fused"], 4), "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
            "tiled_ms": round(med["tiled"], 4), "tiled_ms_min_max": [round(min(ms["tiled"]), 4), round(max(ms["tiled"]), 4)],
            "tiled_over_fused": round(med["tiled"] / med["fused"], 3),
            "fused_us_per_step": round(1e3 * med["fused"] / H, 3), "tiled_us_per_step": round(1e3 * med["tiled"] / H, 3),
            "indicative": bool(med["fused"] < 10.0), "same_shapes": same_shapes,
            "fused_best_length_min": int(a[3].min()), "tiled_lengths_min": int(b[3]),
        }), flush=True)
        eng.close()
        big.close()


if __name__ == "__main__":
    main()
