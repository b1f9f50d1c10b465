"""The planner entry points' refusals that need no handle, pinned to their text: emei_evaluate_sequences, emei_sample_candidates,
emei_sample_candidates_sigma, emei_plan_shooting, emei_plan_mppi, emei_plan_cem and the *_workspace_bytes functions
(emei_mpc_mppi itself has tests/test_mpc_api.py).  Every call has a NULL handle and exactly one bad argument (or none: the handle is then
what is named); the return code and the whole emei_last_error() string are compared with the literals below, so a change of the
host plumbing that moves a check, rewords it or formats a value differently fails here, without a GPU."""
import ctypes as C

import pytest

from emei_amd import _lib

INF = float("inf")
NAN = float("nan")
H, K = 3, 5
_BUF = (C.c_double * 64)()
P = C.cast(_BUF, C.c_void_p)  # never dereferenced: every call here returns before the handle is used


def _evaluate(lib, horizon=H, k=K, discount=1.0, **_):
    return lib.emei_evaluate_sequences(None, horizon, k, P, _lib.ACT_U8, discount, None, P, P, None, None)


def _sample(lib, horizon=H, k=K, **_):
    return lib.emei_sample_candidates(None, horizon, k, 7, None, 0.5, P, _lib.ACT_U8, None)


def _sample_sigma(lib, horizon=H, k=K, **_):
    return lib.emei_sample_candidates_sigma(None, horizon, k, 7, P, P, P, _lib.ACT_F32, None)


def _shooting(lib, horizon=H, k=K, discount=1.0, **_):
    return lib.emei_plan_shooting(None, horizon, k, 7, None, 0.5, discount, None, P, P, _lib.ACT_U8, None, P, P, None, None)


def _mppi(lib, horizon=H, k=K, discount=1.0, temperature=1.0, **_):
    return lib.emei_plan_mppi(None, horizon, k, 7, None, 0.5, discount, temperature, None, P, P, P, P, None, None)


def _cem(lib, horizon=H, k=K, discount=1.0, n_elites=2, **_):
    return lib.emei_plan_cem(None, horizon, k, n_elites, 7, None, 0.5, None, discount, None, P, P, None, P, P, None, None)


# (entry point, its call, the arguments it has beyond horizon / n_candidates)
ENTRY = {
    "emei_evaluate_sequences": (_evaluate, ("discount",)),
    "emei_sample_candidates": (_sample, ()),
    "emei_sample_candidates_sigma": (_sample_sigma, ()),
    "emei_plan_shooting": (_shooting, ("discount",)),
    "emei_plan_mppi": (_mppi, ("discount", "temperature")),
    "emei_plan_cem": (_cem, ("discount", "n_elites")),
}
# one bad argument -> the message behind "<entry point>: "
BAD = [
    ("horizon", {"horizon": 0}, "horizon=0 < 1"),
    ("n_candidates", {"k": 0}, "n_candidates=0 < 1"),
    ("discount", {"discount": 0.0}, "discount=0 is outside (0, 1]"),
    ("discount", {"discount": NAN}, "discount=nan is outside (0, 1]"),
    ("temperature", {"temperature": 0.0}, "temperature=0 must be finite and > 0"),
    ("temperature", {"temperature": INF}, "temperature=inf must be finite and > 0"),
    ("n_elites", {"n_elites": 0}, "n_elites=0 is outside [1, n_candidates=5]"),
    ("n_elites", {"n_elites": K + 1}, "n_elites=6 is outside [1, n_candidates=5]"),
    (None, {}, "null handle"),
]
CALLS = [(fn, kw, f"{fn}: {text}") for fn, (_, has) in ENTRY.items() for arg, kw, text in BAD
         if arg in (None, "horizon", "n_candidates") or arg in has]


@pytest.mark.parametrize("fn,kw,message", CALLS, ids=[f"{fn}-{'-'.join(f'{a}={v}' for a, v in kw.items()) or 'good'}" for fn, kw, _ in CALLS])
def test_null_handle_call(fn, kw, message):
    lib = _lib.lib()
    rc = ENTRY[fn][0](lib, **kw)
    assert (rc, lib.emei_last_error().decode()) == (_lib.ERR_INVALID, message)


def test_the_table_is_whole():
    """6 entry points x (horizon, n_candidates, the all-good call) + discount x 2 on four + temperature x 2 + n_elites x 2"""
    assert len(CALLS) == 6 * 3 + 4 * 2 + 2 + 2


# sizeof(PlanPartial) = 16: one record per (wave, env) segment bound, (n * k + 63) / 64 + n of them; then 8 bytes per candidate
WORKSPACE = {
    "emei_plan_shooting_workspace_bytes": lambda n, k: 16 * ((n * k + 63) // 64 + n),
    "emei_plan_mppi_workspace_bytes": lambda n, k: 16 * ((n * k + 63) // 64 + n) + 8 * n * k,
    "emei_plan_cem_workspace_bytes": lambda n, k: 16 * ((n * k + 63) // 64 + n) + 8 * n * k,
    "emei_mpc_mppi_workspace_bytes": lambda n, k: 8 * n * k,  # shares the shape check (its values: tests/test_mpc_api.py)
}
SHAPES = [
    ((2, 0), "n_candidates=0 < 1"),
    ((2, 2**30), "n_envs * n_candidates = 2147483648 exceeds 2^31 - 1"),
    ((2**31, 1), "n_envs=2147483648"),
]


@pytest.mark.parametrize("fn", sorted(WORKSPACE))
def test_workspace_bytes(fn):
    lib = _lib.lib()
    f = getattr(lib, fn)
    for shape, text in SHAPES:
        assert (f(*shape), lib.emei_last_error().decode()) == (_lib.ERR_INVALID, f"{fn}: {text}"), shape
    for n, k in ((2, 5), (1, 1), (3, 64), (65, 13), (1, 2**31 - 1)):
        assert f(n, k) == WORKSPACE[fn](n, k), (n, k)
    assert lib.emei_plan_shooting_workspace_bytes(2, 5) == 48 and lib.emei_plan_mppi_workspace_bytes(2, 5) == 128
