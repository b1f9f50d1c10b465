"""The planner entry points' refusals that need a handle, pinned to their code and text, and one valid call of each behind them.

Three handles of n_envs = 2: CartPoleSwingUp (discrete, the 4-state kernels), ReboundInvertedPendulumBalancing (continuous, the
4-state kernels) and HopperRunning (the body kernels).  Every refusal below returns before a launch, so nothing runs on the device
for it; the raw C ABI is called so that NULL pointers and wrong dtypes, which Engine refuses itself, reach the library.  The valid
calls at H = 3, K = 5 go through the definition checks of tests/test_gpu_shooting.py, test_gpu_mppi.py, test_gpu_cem.py and
test_gpu_mpc.py (bit for bit against evaluate_sequences(sample_candidates(...)) where those are): a launch descriptor that loses a
field between the entry point and the kernel fails here in seconds."""
import pytest

from emei_amd import _lib
from test_gpu_mppi import CH, _engine, _nominal, _start

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, K = 3, 5
INV, STATE, UNSUPPORTED = _lib.ERR_INVALID, _lib.ERR_STATE, _lib.ERR_UNSUPPORTED
NAN = float("nan")
OVERFLOW = "n_envs * n_candidates = 4294967294 exceeds 2^31 - 1"  # n_envs = 2, n_candidates = 2^31 - 1
DISCRETE_DTYPE = "discrete-action envs take uint8/int32/int64 actions [n]"
SIGMA0 = "sigma=0 with a nominal sequence must be finite and > 0"
SIGMA_NAN = "sigma=nan with a nominal sequence must be finite and > 0"
MPC_ON_BODY = ("emei_mpc_mppi: this handle steps on the body kernels (a multi-body env, or an InvertedPendulum with a non-euler "
               "integrator or observation noise); the fused controller serves the 4-state kernels only")
WHOLE = ("emei_", "discrete-action", "continuous-action", "bad action_dtype")  # messages given whole, not behind "<entry point>: "
KINDS = {"cartpole": ("CartPoleSwingUp", {}), "invpend": ("ReboundInvertedPendulumBalancing", {}), "hopper": ("HopperRunning", CH)}


def _continuous_dtype(eng):
    return f"continuous-action envs take float32 actions [n,{eng.act_dim}]"


class Handle:
    """an engine and 16 separate 4 KiB device buffers, enough for every array of a call at n_envs = 2, H = 3, K = 5"""

    def __init__(self, kind, reset=True):
        name, kw = KINDS[kind]
        self.eng = _engine(name, 2, **kw)
        if reset:
            self.eng.reset(seed=3)
        self.buf = torch.zeros((16, 512), dtype=torch.float64, device=self.eng.device)
        self.good = _lib.ACT_F32 if self.eng.act_dim else _lib.ACT_U8  # an action dtype the env's kind takes
        self.wrong = _lib.ACT_U8 if self.eng.act_dim else _lib.ACT_F32

    def p(self, i):
        return self.buf[i].data_ptr()

    def defaults(self, fn):
        """the arguments of a valid call of `fn` between the handle and the stream, in the ABI's order"""
        p, dt = self.p, self.good
        return {
            "emei_evaluate_sequences": dict(horizon=H, k=K, actions=p(0), dtype=dt, discount=1.0, start=None, ret=p(1), length=p(2),
                                            final=None),
            "emei_sample_candidates": dict(horizon=H, k=K, seed=7, nominal=None, sigma=0.5, out=p(0), dtype=dt),
            "emei_sample_candidates_sigma": dict(horizon=H, k=K, seed=7, nominal=p(1), sigma_map=p(2), out=p(0), dtype=dt),
            "emei_plan_shooting": dict(horizon=H, k=K, seed=7, nominal=None, sigma=0.5, discount=1.0, start=None, ws=p(0), act=p(1),
                                       dtype=dt, seq=None, ret=p(2), idx=p(3), length=None),
            "emei_plan_mppi": dict(horizon=H, k=K, seed=7, nominal=None, sigma=0.5, discount=1.0, temperature=1.0, start=None, ws=p(0),
                                   out=p(1), ret=p(2), idx=p(3), ess=None),
            "emei_plan_cem": dict(horizon=H, k=K, n_elites=2, seed=7, nominal=None, sigma=0.5, sigma_map=None, discount=1.0, start=None,
                                  ws=p(0), mean=p(1), std=None, ret=p(2), idx=p(3), elite=None),
            "emei_mpc_mppi": dict(n_steps=2, horizon=H, k=K, seed=7, nominal=p(0), sigma=0.5, discount=1.0, temperature=1.0, refill=0.5,
                                  lo=-1.0, hi=1.0, ws=p(1), act=p(2), dtype=dt, obs=p(3), rew=p(4), done=p(5), plan_return=None, ess=None,
                                  flags=0),
        }[fn]

    def call(self, fn, **over):
        args = self.defaults(fn)
        assert set(over) <= set(args), (fn, over)
        args.update(over)
        lib = _lib.lib()
        rc = getattr(lib, fn)(self.eng._h, *args.values(), None)
        return rc, lib.emei_last_error().decode()

    def refused(self, fn, code, text, **over):
        if not text.startswith(WHOLE):
            text = f"{fn}: {text}"
        assert self.call(fn, **over) == (code, text), (self.eng.env_name, fn, over)

    def accepted(self, fn, **over):
        rc, msg = self.call(fn, **over)
        torch.cuda.synchronize()
        assert rc == _lib.OK, (self.eng.env_name, fn, over, msg)


@pytest.fixture(scope="module")
def handles():
    return {kind: Handle(kind) for kind in KINDS}


CANDIDATE_FNS = ("emei_sample_candidates", "emei_sample_candidates_sigma", "emei_plan_shooting", "emei_plan_mppi", "emei_plan_cem")
ALL_FNS = ("emei_evaluate_sequences",) + CANDIDATE_FNS + ("emei_mpc_mppi",)
WITH_DTYPE = ("emei_evaluate_sequences", "emei_sample_candidates", "emei_sample_candidates_sigma", "emei_plan_shooting", "emei_mpc_mppi")
WITH_SIGMA = ("emei_sample_candidates", "emei_plan_shooting", "emei_plan_mppi", "emei_plan_cem", "emei_mpc_mppi")
WITH_START = ("emei_evaluate_sequences", "emei_plan_shooting", "emei_plan_mppi", "emei_plan_cem")


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_too_many_candidates(handles, kind):
    h = handles[kind]
    for fn in ALL_FNS:
        h.refused(fn, INV, OVERFLOW, k=2**31 - 1)
    # horizon * act_dim words of a candidate's stream
    if h.eng.act_dim == 3:
        h.refused("emei_sample_candidates", INV, "horizon * act_dim exceeds 2^31 - 1", horizon=2**30)
        h.refused("emei_plan_mppi", INV, "horizon * act_dim exceeds 2^31 - 1", horizon=2**30)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_wrong_action_dtype(handles, kind):
    h = handles[kind]
    text = _continuous_dtype(h.eng) if h.eng.act_dim else DISCRETE_DTYPE
    for fn in WITH_DTYPE:
        h.refused(fn, INV, text, dtype=h.wrong)
        h.refused(fn, INV, "bad action_dtype 7", dtype=7)
        h.refused(fn, INV, "bad action_dtype -1", dtype=-1)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_sigma_with_a_nominal(handles, kind):
    h = handles[kind]
    for fn in WITH_SIGMA:
        if fn == "emei_mpc_mppi" and kind == "hopper":
            continue  # below: the body kernels have no fused controller
        for sigma, text in ((0.0, SIGMA0), (-1.0, "sigma=-1 with a nominal sequence must be finite and > 0"), (NAN, SIGMA_NAN),
                            (float("inf"), "sigma=inf with a nominal sequence must be finite and > 0")):
            if h.eng.act_dim:
                h.refused(fn, INV, text, nominal=h.p(6), sigma=sigma)
            else:  # the discrete envs' nominal is a probability: sigma is not read
                h.accepted(fn, nominal=h.p(6), sigma=sigma)
        h.accepted(fn, nominal=h.p(6), sigma=0.5)
        if fn != "emei_mpc_mppi":
            h.accepted(fn, nominal=None, sigma=0.0)  # without a nominal sigma does not count
    if h.eng.act_dim:
        # with a sigma_map the scalar does not count either
        h.accepted("emei_plan_cem", nominal=h.p(6), sigma=0.0, sigma_map=h.p(7), std=h.p(8))
        h.accepted("emei_plan_cem", nominal=h.p(6), sigma=NAN, sigma_map=h.p(7), std=h.p(8))


def test_mpc_mppi_always_plans_around_a_nominal(handles):
    """its sigma counts even when the nominal is the NULL the call refuses a few checks later"""
    c, d, b = handles["invpend"], handles["cartpole"], handles["hopper"]
    c.refused("emei_mpc_mppi", INV, SIGMA0, nominal=None, sigma=0.0)
    c.refused("emei_mpc_mppi", INV, SIGMA_NAN, nominal=None, sigma=NAN)
    c.refused("emei_mpc_mppi", INV, "null nominal", nominal=None)
    d.refused("emei_mpc_mppi", INV, "null nominal", nominal=None, sigma=0.0)
    b.refused("emei_mpc_mppi", INV, SIGMA0, nominal=None, sigma=0.0)
    b.refused("emei_mpc_mppi", UNSUPPORTED, MPC_ON_BODY)
    for h in (c, d, b):
        h.refused("emei_mpc_mppi", INV, "unknown flags 0x2", flags=2)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_null_pointers(handles, kind):
    h = handles[kind]
    for arg in ("actions", "ret", "length"):
        h.refused("emei_evaluate_sequences", INV, "null argument", **{arg: None})
    h.refused("emei_sample_candidates", INV, "null argument", out=None)
    for arg in ("ws", "act", "ret", "idx"):
        h.refused("emei_plan_shooting", INV, "null argument", **{arg: None})
    h.refused("emei_plan_mppi", INV, "null workspace", ws=None)
    h.refused("emei_plan_mppi", INV, "null nominal_out", out=None)
    h.refused("emei_plan_cem", INV, "null workspace", ws=None)
    h.refused("emei_plan_cem", INV, "null mean_out", mean=None)
    h.refused("emei_mpc_mppi", INV, "null nominal", nominal=None)
    h.refused("emei_mpc_mppi", INV, "null workspace", ws=None)
    h.refused("emei_mpc_mppi", INV, "null actions_out", act=None)
    if h.eng.act_dim:
        h.refused("emei_sample_candidates_sigma", INV, "null argument", out=None)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_sigma_map(handles, kind):
    h = handles[kind]
    h.refused("emei_plan_cem", INV, "a sigma_map needs a nominal", sigma_map=h.p(7))
    if h.eng.act_dim:
        h.refused("emei_sample_candidates_sigma", INV, "null nominal or sigma_map", nominal=None)
        h.refused("emei_sample_candidates_sigma", INV, "null nominal or sigma_map", sigma_map=None)
        h.accepted("emei_sample_candidates_sigma")
    else:
        text = "a discrete env takes no sigma_map and has no std_out"
        h.refused("emei_plan_cem", INV, text, nominal=h.p(6), sigma_map=h.p(7))
        h.refused("emei_plan_cem", INV, text, std=h.p(8))
        h.refused("emei_sample_candidates_sigma", INV, "a discrete env takes no sigma_map")
        h.refused("emei_sample_candidates_sigma", INV, "a discrete env takes no sigma_map", nominal=None, sigma_map=None, out=None)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_before_reset(handles, kind):
    h = Handle(kind, reset=False)
    text = "call reset before using the state"
    for fn in WITH_START:
        h.refused(fn, STATE, text)
        h.refused(fn, INV, OVERFLOW, k=2**31 - 1)  # the state is the last thing looked at
    h.refused("emei_evaluate_sequences", INV, "null argument", ret=None)
    h.refused("emei_plan_shooting", INV, "null argument", ret=None)
    h.refused("emei_plan_mppi", INV, "null nominal_out", out=None)
    h.refused("emei_plan_cem", INV, "null mean_out", mean=None)
    h.refused("emei_mpc_mppi", STATE, text)  # before the kernel family is looked at: the Hopper's handle too
    h.refused("emei_mpc_mppi", INV, "null actions_out", act=None)
    # the sampling calls read no state
    h.accepted("emei_sample_candidates")
    if h.eng.act_dim:
        h.accepted("emei_sample_candidates_sigma")
    # with start rows the handle's state is not needed
    st = handles[kind].eng.get_state()
    for fn in ("emei_plan_shooting", "emei_plan_mppi", "emei_plan_cem"):
        h.accepted(fn, start=st.data_ptr())


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_order_of_refusals(handles, kind):
    """a call that is bad in two ways names the earlier check: the scalars, the handle, sigma, the candidate count, the dtype, the
    call's own pointers, the device, the state"""
    h = handles[kind]
    e = h.eng
    dtype_text = _continuous_dtype(e) if e.act_dim else DISCRETE_DTYPE
    # emei_evaluate_sequences: scalars, null arguments, the count, the dtype
    h.refused("emei_evaluate_sequences", INV, "discount=2 is outside (0, 1]", discount=2.0, ret=None, k=2**31 - 1)
    h.refused("emei_evaluate_sequences", INV, "null argument", ret=None, k=2**31 - 1, dtype=h.wrong)
    h.refused("emei_evaluate_sequences", INV, OVERFLOW, k=2**31 - 1, dtype=h.wrong)
    # the calls that draw candidates
    for fn in CANDIDATE_FNS + ("emei_mpc_mppi",):
        args = h.defaults(fn)
        out = {"emei_sample_candidates": "out", "emei_sample_candidates_sigma": "out", "emei_plan_shooting": "ws", "emei_plan_mppi": "ws",
               "emei_plan_cem": "ws", "emei_mpc_mppi": "ws"}[fn]
        h.refused(fn, INV, "horizon=0 < 1", horizon=0, k=2**31 - 1, **{out: None})
        if "discount" in args:
            h.refused(fn, INV, "discount=0 is outside (0, 1]", discount=0.0, k=2**31 - 1, **{out: None})
        if "sigma" in args and e.act_dim:
            h.refused(fn, INV, SIGMA0, nominal=h.p(6), sigma=0.0, k=2**31 - 1, **{out: None})
        if "dtype" in args:
            h.refused(fn, INV, OVERFLOW, k=2**31 - 1, dtype=h.wrong, **{out: None})
            h.refused(fn, INV, dtype_text, dtype=h.wrong, **{out: None})
        else:
            h.refused(fn, INV, OVERFLOW, k=2**31 - 1, **{out: None})
    h.refused("emei_plan_mppi", INV, "temperature=0 must be finite and > 0", temperature=0.0, ws=None)
    h.refused("emei_plan_mppi", INV, "null workspace", ws=None, out=None)
    h.refused("emei_plan_cem", INV, "n_elites=6 is outside [1, n_candidates=5]", n_elites=6, discount=0.0)
    h.refused("emei_plan_cem", INV, "a sigma_map needs a nominal", sigma_map=h.p(7), std=h.p(8), ws=None)
    h.refused("emei_plan_cem", INV, "null workspace", ws=None, mean=None)
    if not e.act_dim:
        h.refused("emei_plan_cem", INV, "a discrete env takes no sigma_map and has no std_out", std=h.p(8), ws=None)
        h.refused("emei_sample_candidates_sigma", INV, DISCRETE_DTYPE, dtype=h.wrong)
    else:
        h.refused("emei_sample_candidates_sigma", INV, "null nominal or sigma_map", nominal=None, out=None)
    # emei_mpc_mppi: the dtype, the flags, nominal, workspace, actions_out, (the state,) the kernel family
    h.refused("emei_mpc_mppi", INV, "horizon=257 exceeds EMEI_MPC_MAX_HORIZON=256 (the nominal lives in LDS)", horizon=257, k=2**31 - 1)
    h.refused("emei_mpc_mppi", INV, dtype_text, dtype=h.wrong, flags=2)
    h.refused("emei_mpc_mppi", INV, "unknown flags 0x2", flags=2, nominal=None)
    h.refused("emei_mpc_mppi", INV, "null nominal", nominal=None, ws=None)
    h.refused("emei_mpc_mppi", INV, "null workspace", ws=None, act=None)


# ------------------------------------------------------------------------------------------------ one valid call of each
# the candidates: None = fair coins / uniform, "scalar" = a nominal with one sigma, "map" = a nominal with a sigma per entry
@pytest.mark.parametrize("kind,mode", [(k, m) for k in sorted(KINDS) for m in (None, "scalar", "map") if (k, m) != ("cartpole", "map")])
def test_valid_calls_equal_their_definitions(handles, kind, mode):
    """plan_shooting, plan_mppi and plan_cem from the handle's state and from start rows, with each way of drawing candidates"""
    import test_gpu_cem
    import test_gpu_mppi
    import test_gpu_shooting

    eng = handles[kind].eng
    nom, sigma = _nominal(eng, H, seed=K) if mode else (None, None)
    for st in (None, _start(eng)):
        test_gpu_shooting._check_definition(eng, H, K, 11, 0.99, nominal=nom, sigma=sigma, start_state=st)
        test_gpu_mppi._check_definition(eng, H, K, 11, 0.99, nominal=nom, sigma=sigma, start_state=st)
        smap = test_gpu_cem._sigma_map(eng, nom, seed=K + 1) if mode == "map" else sigma
        test_gpu_cem._check_definition(eng, H, K, 2, 11, 0.99, nominal=nom, sigma=smap, start_state=st)
    assert eng.solver_cap_hits() == 0


@pytest.mark.parametrize("name,sigma", [("CartPoleSwingUp", None), ("ReboundInvertedPendulumBalancing", 0.5)])
def test_valid_mpc_mppi_equals_the_loop(name, sigma):
    import test_gpu_mpc as T

    fused, loop = T._pair(name, 2)
    a, b = T._run_both(fused, loop, 2, H, K, T._state0(fused), sigma=sigma, discount=0.97)
    T._assert_equal(a, b, name)
