"""The kernel matrix: one record per compiled dynamics configuration of libemei_hip.so, and the fused entry points each must serve.

emei_amd/csrc/Makefile compiles 16 four-state translation units (TUS) and 24 body translation units (BODIES); every body unit is
instantiated once with RK4 = false and once with RK4 = true, which makes 16 + 2 * 24 = 64 configurations (ROWS).  Every fused entry
point (ENTRY_POINTS) is a kernel template instantiated again for each of them.  tests/test_kernel_matrix.py holds this table to the
Makefile and to body_dispatch.hip and shows from the CPU oracle alone that the start states do what they promise;
tests/test_gpu_kernel_matrix.py launches every (entry point, row) pair.  A new translation unit or entry point must be added here.

A helper module: no fixtures, no test, and nothing here touches a GPU."""
import numpy as np

import plan_reference as PR

PRECISIONS = {"ref": "f64", "f32": "f32"}
IP = ["ReboundInvertedPendulumBalancing", "BoundaryInvertedPendulumBalancing", "ReboundInvertedPendulumSwingUp",
      "BoundaryInvertedPendulumSwingUp"]  # ip0 .. ip3 (pendulum_dispatch.hip / body_dispatch.hip)
DP = ["ReboundInvertedDoublePendulumBalancing", "BoundaryInvertedDoublePendulumBalancing", "ReboundInvertedDoublePendulumSwingUp",
      "BoundaryInvertedDoublePendulumSwingUp"]  # dp0 .. dp3
CP = ["CartPoleSwingUp", "CartPoleBalancing"]  # cp0 / cr0, cp1 / cr1
# enum emei_env_id as body_dispatch.hip spells it
ENUM = {"HalfCheetahRunning": "EMEI_HALFCHEETAH_RUNNING", "HopperRunning": "EMEI_HOPPER_RUNNING"}
for _names, _tag in ((IP, "IP"), (DP, "IDP")):
    for _n, _suffix in zip(_names, ("REBOUND_BALANCING", "BOUNDARY_BALANCING", "REBOUND_SWINGUP", "BOUNDARY_SWINGUP")):
        ENUM[_n] = f"EMEI_{_tag}_{_suffix}"

# emei_last_rollout_kernel of a rollout at the matrix's shapes: a ragged N takes the generic four-state kernel with all three outputs, a
# body handle its one-piece rollout kernel (_lib is plain Python: it loads the library only when asked to)
from emei_amd._lib import KERNEL_BODY, KERNEL_BODY_RK4, KERNEL_PEND_GENERIC_FULL  # noqa: E402

RAIL = {"ip": 2.0, "dp": 3.0}  # the slider's range (inverted_pendulum.xml / inverted_double_pendulum.xml)
# ids whose terminal function can say yes on finite rows (oracle/emei_oracle.c: cp_terminal, ip_terminal; dpend_oracle.c)
TERMINATING = set(CP) | {IP[0], IP[1], IP[3], DP[0], DP[1], DP[3]}


class Row:
    """One compiled configuration.  kw: Engine keyword arguments (precision, integrator / ode_method, solver, freq_rate and
    real_time_scale as the family's tests use them); tu: its object in the Makefile; rk4: the body unit's RK4 instantiation;
    kernel: the emei_last_rollout_kernel id of a rollout; extra: a layer-1-only row (semi-implicit Euler is a runtime flag of the
    non-RK4 kernel)."""

    def __init__(self, env, family, kw, tu, rk4=False, extra=False):
        self.env, self.family, self.kw, self.tu, self.rk4, self.extra = env, family, kw, tu, rk4, extra
        self.body = tu.startswith("body_tu_")
        self.kernel = (KERNEL_BODY_RK4 if rk4 else KERNEL_BODY) if self.body else KERNEL_PEND_GENERIC_FULL
        how = kw.get("ode_method") if family == "cartpole" else kw.get("integrator", "euler")
        self.id = "-".join([tu.split("_tu_")[1], {"semi_implicit_euler": "semi"}.get(how, how)])
        self.seed = SEEDS.get(family, 0)

    # -- the oracle -------------------------------------------------------------------------------
    def opts(self):
        from oracle import oracle as O

        return O.opts(self.kw.get("integrator", "euler"), solver=self.kw.get("solver", "newton"))

    def oracle_step(self, s0, act, freq_rate=None):
        """one env-step of the CPU oracle -> (next state, observation, reward, terminal); act as the device reads it"""
        from oracle import oracle as O

        fr, dt = int(freq_rate or self.kw["freq_rate"]), self.kw["real_time_scale"]
        variant = PR.FAMILY[self.env][1]
        if self.family == "cartpole":
            st, rew, term = O.cartpole_step(variant, s0, act, fr, dt, self.kw["ode_method"])
            return st, st, rew, term
        a = np.asarray(act, np.float32).astype(np.float64)
        if self.family in ("ip_staged", "ip"):
            return O.ip_step(variant, s0, a, fr, dt, self.opts())
        if self.family == "dp":
            return O.dpend_step(variant, s0, a, fr, dt, self.opts())
        step = O.cheetah_step if self.family == "cheetah" else O.hopper_step
        st, rew, term = step(s0, a, fr, dt, self.opts())
        return st, st, rew, term

    # -- inputs -----------------------------------------------------------------------------------
    def states(self, n, seed=None):
        """start rows [n, state_dim] float64 that activate the family's constraints (see the generators below)"""
        return GENERATORS[self.family](self, n, np.random.default_rng(self.seed if seed is None else seed))

    def actions(self, n, seed=None, lead=()):
        """actions lead + [n(, act_dim)] as step() takes them, beyond the ctrlrange so that the clip is exercised"""
        rng = np.random.default_rng(1000 + (self.seed if seed is None else seed))
        if self.family == "cartpole":
            return rng.integers(0, 2, lead + (n,)).astype(np.int64)
        amp, tail = {"ip_staged": (3.5, ()), "ip": (3.5, ()), "dp": (1.3, ()), "cheetah": (1.3, (6,)), "hopper": (1.3, (3,))}[self.family]
        return rng.uniform(-amp, amp, lead + (n,) + tail).astype(np.float32)

    def constraint_active(self, s0):
        """[n] bool: the rows of s0 on which the family's constraint rows exist (None for CartPole, which has none)"""
        from oracle import oracle as O

        if self.family in ("ip_staged", "ip", "dp"):
            return np.abs(s0[:, 0]) > RAIL["dp" if self.family == "dp" else "ip"]
        if self.family in ("cheetah", "hopper"):
            return O.planar_row_mask(self.family, s0) != 0
        return None

    # -- the float32 one-step comparison -------------------------------------------------------------
    def f32_bound(self):
        """(tolerance, floor, quantities) that the family's own float32 one-step test asserts"""
        if self.family == "cartpole":  # test_gpu_cartpole.py:42-44; test_gpu_cartpole_rk4.py:55 (the observation only)
            return 1e-4, 1.0, ("obs", "reward") if self.kw["ode_method"] == "euler" else ("obs",)
        if self.family in ("ip_staged", "ip"):  # test_gpu_invpend.py:52-54
            return 2e-4, 1.0, ("obs", "reward")
        if self.family == "dp":  # test_gpu_dpend.py:50
            return 2e-3, 1e-3, ("obs",)
        return 5e-3, 1e-3, ("obs",)  # test_gpu_cheetah.py:50, test_gpu_hopper.py:91

    def f32_rows(self, n):
        """[n] bool: the rows a float32 one-step comparison of this family covers.  The Hopper's float32 test (test_gpu_hopper.py:
        85-91) leaves the stiff limit / deep-contact rows of its draw out (index % 5 < 2); the capsule-pair rows that _hopper_states
        appends (the last quarter, the ragged wave among them) are all covered."""
        idx = np.arange(n)
        if self.family != "hopper":
            return np.ones(n, bool)
        return ((idx % 5) >= 2) | (idx >= n - n // 4)

    def ill_conditioned(self, s0, act, freq_rate, bound, floor, amp=1e-5):
        """[n] bool: rows on which the ORACLE's own next state moves by more than `bound` (relative, with `floor`) when the start
        state moves by `amp` relative — every coordinate alone, both ways, and eight fixed sign patterns of all of them.  1e-5 is
        what float32 arithmetic amounts to on this family (the measured float32 errors of its well-conditioned rows are a few
        1e-5); on such a row a constraint row switches on or off inside the step, and no float32 kernel can be held to `bound`
        there.  The one-step counterpart of plan_reference.undecidable; its share is capped in tests/test_kernel_matrix.py."""
        st = self.oracle_step(s0, act, freq_rate)[0]
        D = s0.shape[1]
        rng = np.random.default_rng(7)
        patterns = [sgn * np.eye(D)[d] for d in range(D) for sgn in (1.0, -1.0)] + [rng.choice([-1.0, 1.0], D) for _ in range(8)]
        worst = np.zeros(len(s0))
        for p in patterns:
            moved = self.oracle_step(s0 * (1.0 + amp * p), act, freq_rate)[0]
            worst = np.maximum(worst, (np.abs(moved - st) / np.maximum(np.abs(st), floor)).max(axis=1))
        return worst > bound

    def __repr__(self):
        return f"Row({self.id})"


# ------------------------------------------------------------------------------------------------ start-state generators
def _cartpole_states(row, n, rng):
    """plan_reference's reset rows, a third of them spread across the terminal thresholds (|x| = 5 / 2.4, |theta| = 12 degrees)"""
    s0, _ = PR.BUILDERS["cartpole"](row.env, n, 1, 1, int(rng.integers(1 << 30)))
    k = n // 3
    thr = 5.0 if row.env == "CartPoleSwingUp" else 2.4
    s0[:k, 0] = rng.uniform(-1.2 * thr, 1.2 * thr, k)
    s0[:k, 1] = rng.normal(0, 1.0, k)
    s0[:k, 2] += rng.uniform(-0.4, 0.4, k)
    s0[:k, 3] = rng.normal(0, 1.0, k)
    return s0


def _ip_states(row, n, rng):
    """test_gpu_invpend._states (the cart beyond the +-2 rail) with an eighth of the rows at the hinge stop of +-90 degrees"""
    from start_states import invpend_states as _states

    s = _states(rng, n)
    k = n // 8
    s[n // 4: n // 4 + k, 1] = rng.choice([-1.0, 1.0], k) * (np.pi / 2 + rng.uniform(-0.1, 0.15, k))
    return s


def _dp_states(row, n, rng):
    """the draw of test_gpu_dpend.py:35-36: the cart beyond the +-3 rail, a quarter of the rows near upright"""
    s0 = np.column_stack([rng.uniform(-3.2, 3.2, n), rng.uniform(-6, 6, (n, 2)), rng.normal(0, 1.5, n), rng.normal(0, 3, (n, 2))])
    s0[: n // 4] = rng.standard_normal((n // 4, 6)) * 5e-3
    return s0


def _cheetah_states(row, n, rng):
    from start_states import cheetah_states as _states

    return _states(rng, n)  # crouched into the floor, joints past their limits


def _hopper_states(row, n, rng):
    """test_gpu_hopper._states (floor contact, joint limits) with a quarter of the rows folded as test_capsule_pairs_vs_oracle folds
    them: capsule-pair rows"""
    from start_states import hopper_states as _states

    s = _states(rng, n)
    k = n // 4
    q = np.concatenate([rng.normal(0, 0.3, (k, 1)), rng.uniform(0.1, 2.5, (k, 1)), rng.normal(0, 1.2, (k, 1)),
                        rng.uniform(-2.9, -0.9, (k, 1)), rng.uniform(-2.9, -1.4, (k, 1)), rng.uniform(-0.9, 0.9, (k, 1))], axis=1)
    s[n - k:] = np.concatenate([q, rng.normal(0, 2.0, (k, 6))], axis=1)
    return s


GENERATORS = {"cartpole": _cartpole_states, "ip_staged": _ip_states, "ip": _ip_states, "dp": _dp_states, "cheetah": _cheetah_states,
              "hopper": _hopper_states}

# seeds of the start rows, chosen on the CPU so that at the layer-1 shape (130 rows, freq_rate 2) every promise of
# tests/test_kernel_matrix.py holds: at most 1 % of a row's terminal flags undecidable at the observation tolerance
# (plan_reference.undecidable), at most 1 % of the Hopper's float32 rows ill-conditioned (Row.ill_conditioned).  By family; a family that
# is not listed uses seed 0 (the double pendulum's draw 0 puts under 5 % of the carts beyond the rail; the Hopper's draws 0 .. 29 each
# hold two or more ill-conditioned rows in some configuration)
SEEDS = {"dp": 2, "hopper": 30}

MUJOCO = dict(PR.MUJOCO)  # freq_rate 4, real_time_scale 0.002
PEND = dict(freq_rate=4, real_time_scale=0.02)  # test_gpu_invpend.py:38, test_gpu_dpend.py:28


def _build():
    rows = []
    for prec, p in PRECISIONS.items():
        for v, env in enumerate(IP):  # the staged InvertedPendulum: Euler, no noise
            rows.append(Row(env, "ip_staged", dict(PEND, precision=prec), f"pend_tu_ip{v}_{p}"))
        for v, env in enumerate(CP):
            for method, tag in (("euler", "cp"), ("rk4", "cr")):
                rows.append(Row(env, "cartpole", dict(freq_rate=1, real_time_scale=0.02, precision=prec, ode_method=method),
                                f"pend_tu_{tag}{v}_{p}"))
        for rk4 in (False, True):
            for v, env in enumerate(IP):  # plain Euler takes the staged kernel: the non-RK4 body row is semi-implicit
                integ = "rk4" if rk4 else "semi_implicit_euler"
                rows.append(Row(env, "ip", dict(PEND, precision=prec, integrator=integ), f"body_tu_ip{v}_{p}", rk4))
            for v, env in enumerate(DP):
                rows.append(Row(env, "dp", dict(PEND, precision=prec, integrator="rk4" if rk4 else "euler"), f"body_tu_dp{v}_{p}", rk4))
            for env, fam, tag in (("HalfCheetahRunning", "cheetah", "ch"), ("HopperRunning", "hopper", "hp")):
                for solver, s in (("newton", ""), ("sweep1", "s")):
                    rows.append(Row(env, fam, dict(MUJOCO, precision=prec, integrator="rk4" if rk4 else "euler", solver=solver),
                                    f"body_tu_{tag}{s}_{p}", rk4))
    extra = [Row(r.env, r.family, dict(r.kw, integrator="semi_implicit_euler"), r.tu, extra=True)
             for r in rows if r.body and not r.rk4 and r.family != "ip"]
    return rows, extra


ROWS, EXTRA_ROWS = _build()
LAYER1_ROWS = ROWS + EXTRA_ROWS
assert len(ROWS) == 64 and len({r.id for r in LAYER1_ROWS}) == len(LAYER1_ROWS)

# ------------------------------------------------------------------------------------------------ the fused entry points
ENTRY_POINTS = ["rollout", "rollout_chunked", "evaluate_sequences", "plan_shooting", "plan_mppi", "plan_cem", "mpc_mppi", "mpc_cem",
                "rollout_policy", "rollout_policy_noisy", "rollout_policy_deep", "evaluate_policies", "evaluate_policies_deep",
                "plan_policy", "plan_policy_deep", "batch_next_obs"]


class Refusal:
    """What an unsupported (entry point, row) pair must do.  raises: the exception and a fragment of the ABI's message.  ignored:
    the call is accepted and the option has no effect (the launch stays on `kernel`).  unreachable: the entry point has no
    argument that selects the row's unit; the test pins what it runs instead."""

    def __init__(self, kind, exc=None, match=None):
        self.kind, self.exc, self.match = kind, exc, match


# (entry point, row predicate, expected refusal), each decided from the ABI's own checks:
UNSUPPORTED = [
    # abi.hip:check_mpc_handle: of the handles that step on the body kernels only the InvertedDoublePendulum has body_mpc_*_kernel
    ("mpc_mppi", lambda r: r.body and r.family != "dp", Refusal("raises", NotImplementedError, "steps on the body kernels")),
    ("mpc_cem", lambda r: r.body and r.family != "dp", Refusal("raises", NotImplementedError, "steps on the body kernels")),
    # body_kernels.h:BODY_OP_NEXT_OBS: DPendBody::kObsIsState is false (the observation's wrap is not invertible)
    ("batch_next_obs", lambda r: r.family == "dp", Refusal("raises", NotImplementedError, "does not determine its state")),
    # abi.hip:emei_next_obs_io builds its BodyLaunch without a solver: the single-sweep units' next-obs kernels cannot be selected
    ("batch_next_obs", lambda r: r.kw.get("solver") == "sweep1", Refusal("unreachable")),
    # abi.hip:emei_create allocates the work queue for steps_as_body handles only; emei_rollout's four-state branch never reads
    # rollout_chunk_steps (tests/test_gpu_chunked_rollout.py:82-86: accepted and unused)
    ("rollout_chunked", lambda r: not r.body, Refusal("ignored")),
    # body_kernels.h:launch_body chunks only the bodies with one-wave rollout blocks (rollout_block<Body>() == kWave); the
    # single-sweep Hopper runs two waves per SIMD in 256-thread blocks (hopper_model.h: kMinWavesPerEU), so the option has no effect
    ("rollout_chunked", lambda r: r.family == "hopper" and r.kw["solver"] == "sweep1", Refusal("ignored")),
]


def refusal(entry, row):
    """the Refusal of an (entry point, row) pair, or None where the pair is served"""
    for e, pred, ref in UNSUPPORTED:
        if e == entry and pred(row):
            return ref
    return None


SUPPORTED = [(e, r) for e in ENTRY_POINTS for r in ROWS if refusal(e, r) is None]
REFUSED = [(e, r) for e in ENTRY_POINTS for r in ROWS if refusal(e, r) is not None]
