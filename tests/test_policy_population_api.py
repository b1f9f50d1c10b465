"""emei_evaluate_policies on the host: declared (additive under ABI 8), exported and bound; the header carries the history line and a
normative comment of its own; every refusal that needs no device comes back EMEI_ERR_INVALID with a message that starts with
`emei_evaluate_policies:` and names the argument, for a NULL handle and before any HIP call (no GPU needed), in the header's order:
horizon, n_policies, discount, the struct pointer, struct_size, hidden, out_mode, reserved, then the handle.  And the host logic of
PolicyPopulation on CPU tensors: stacking, indexing, the shape errors, the pointers and offsets the kernels rely on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "emei_evaluate_policies"


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    proto = re.search(r"EMEI_API\s+int\s+emei_evaluate_policies\s*\(([^;]*)\)\s*;", hdr)
    assert proto
    args = [a.strip() for a in " ".join(proto.group(1).split()).split(",")]
    assert args == ["emei_env* h", "int32_t horizon", "int32_t n_policies", "const emei_policy* stacked", "double discount",
                    "const double* start_state", "double* return_out", "int32_t* length_out", "float* final_obs_out", "void* stream"]
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    assert FN in hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    # a normative comment of its own, between emei_rollout_policy's prototype and this one
    after = hdr[hdr.index("EMEI_API int emei_rollout_policy("):]
    comment = after[:after.index("EMEI_API int emei_evaluate_policies(")]
    for word in ("Start", "Observe", "Policy", "Step and score", "[n_policies, n_envs]", "[n_policies, n_envs, obs_dim]", "Replay", "Sharding",
                 "capturable", "pend_policy_eval_kernel", "body_policy_eval_kernel", "EMEI_ERR_STATE", "EMEI_ERR_INVALID", "emei_set_state",
                 "emei_get_obs", "emei_evaluate_sequences", "emei_rollout_policy", "emei_get_solver_cap_hits", "DEVICE pointers",
                 "[P, hidden, obs_dim]", "[P, n_out, hidden]", "policy-major", "untouched", "lane lending"):
        assert word in comment, word
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert FN in _lib.SYMBOLS and FN in exported and hasattr(lib, FN)
    assert len(_lib.SYMBOLS[FN][1]) == len(args)
    assert lib.emei_abi_version() == 8 and _lib.ABI_VERSION == 8
    # no kernel id of its own: the call does not report through emei_last_rollout_kernel
    assert sorted(_lib.POLICY_KERNEL_NAMES) == [15, 16, 17] and len(_lib.KERNEL_NAMES) == 15


def test_refusals_with_a_null_handle():
    lib = _lib.lib()
    buf = {k: C.cast((C.c_double * 64)(), C.c_void_p) for k in ("w1", "b1", "w2", "b2", "ret", "len", "fo", "start")}
    size = C.sizeof(_lib.EmeiPolicy)

    def call(horizon=3, n_policies=2, stacked=True, struct_size=size, hidden=4, out_mode=0, reserved=0, w1=buf["w1"], b1=buf["b1"],
             w2=buf["w2"], b2=buf["b2"], discount=1.0, ret=buf["ret"], start=None):
        pol = _lib.EmeiPolicy(struct_size, hidden, out_mode, reserved, w1, b1, w2, b2)
        rc = lib.emei_evaluate_policies(None, horizon, n_policies, C.byref(pol) if stacked else None, discount, start, ret, buf["len"],
                                        buf["fo"], None)
        return rc, lib.emei_last_error().decode()

    rc, msg = call()
    assert rc == _lib.ERR_INVALID and msg.startswith(FN + ":") and "null handle" in msg, msg
    nan = float("nan")
    cases = (({"horizon": 0}, "horizon"), ({"horizon": -5}, "horizon"), ({"n_policies": 0}, "n_policies"), ({"n_policies": -1}, "n_policies"),
             ({"discount": 0.0}, "discount"), ({"discount": -0.5}, "discount"), ({"discount": 1.0000001}, "discount"), ({"discount": nan}, "discount"),
             ({"stacked": False}, "null stacked"),
             ({"struct_size": 0}, "stacked.struct_size"), ({"struct_size": size - 8}, "struct_size"), ({"struct_size": size + 8}, "struct_size"),
             ({"hidden": -1}, "stacked.hidden"), ({"hidden": 1025}, "hidden"), ({"hidden": 2**31 - 1}, "hidden"),
             ({"out_mode": 2}, "stacked.out_mode"), ({"out_mode": -1}, "out_mode"), ({"reserved": 1}, "stacked.reserved"), ({"reserved": -7}, "reserved"))
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith(FN + ":") and word in msg, (kw, rc, msg)
    # the edges pass the checks that need no handle: the handle is what is named
    for kw in ({"hidden": 0}, {"hidden": 1024}, {"out_mode": 1}, {"horizon": 1}, {"horizon": 2**31 - 1}, {"n_policies": 1},
               {"n_policies": 2**31 - 1}, {"discount": 1.0}, {"discount": 5e-324}, {"start": buf["start"]}):
        assert "null handle" in call(**kw)[1], kw
    # in the order of the header
    bad = {"horizon": 0, "n_policies": 0, "discount": 2.0, "stacked": False}
    for key, word in (("horizon", "horizon"), ("n_policies", "n_policies"), ("discount", "discount"), ("stacked", "null stacked")):
        msg = call(**bad)[1]
        assert word in msg and msg.startswith(FN + ":"), (key, msg)
        del bad[key]
    bad = {"struct_size": 1, "hidden": -1, "out_mode": 9, "reserved": 3}
    for key in ("struct_size", "hidden", "out_mode", "reserved"):
        msg = call(**bad)[1]
        assert key in msg and msg.startswith(FN + ":"), (key, msg)
        del bad[key]
    # what comes after the handle (the weights, return_out) does not win over it
    assert "null handle" in call(w1=None, b1=None, w2=None, b2=None, ret=None)[1]
    assert "reserved" in call(reserved=1, w2=None, ret=None)[1]
    with pytest.raises(ValueError, match="n_policies"):
        _lib.check(call(n_policies=0)[0])
    # emei_rollout_policy's messages are what they were (the two calls share their struct checks)
    pol = _lib.EmeiPolicy(size, -1, 0, 0, None, None, None, None)
    assert lib.emei_rollout_policy(None, 3, C.byref(pol), None, 0, None, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.emei_last_error().decode() == "emei_rollout_policy: policy.hidden=-1 is outside [0, EMEI_POLICY_MAX_HIDDEN=1024]"
    assert lib.emei_rollout_policy(None, 3, None, None, 0, None, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.emei_last_error().decode() == "emei_rollout_policy: null policy"
    assert lib.emei_evaluate_sequences(None, 3, 0, None, 0, 1.0, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.emei_last_error().decode() == "emei_evaluate_sequences: n_candidates=0 < 1"


# ---------------------------------------------------------------------------------------------- PolicyPopulation, on CPU tensors
torch = pytest.importorskip("torch")


def _members(P, obs_dim, hidden, n_out, out="clip", seed=0):
    from emei_amd.policy import MLPPolicy

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    if hidden == 0:
        return [MLPPolicy(r(n_out, obs_dim), r(n_out), out=out) for _ in range(P)]
    return [MLPPolicy(r(n_out, hidden), r(n_out), r(hidden, obs_dim), r(hidden), out=out) for _ in range(P)]


@pytest.mark.parametrize("obs_dim,hidden,n_out", [(4, 0, 1), (4, 5, 1), (18, 7, 6), (12, 0, 3)])
def test_stacking_indexing_pointers_and_offsets(obs_dim, hidden, n_out):
    import emei_amd
    from emei_amd.policy import MLPPolicy, PolicyPopulation

    assert emei_amd.PolicyPopulation is PolicyPopulation
    P = 3
    members = _members(P, obs_dim, hidden, n_out, out="tanh")
    pop = PolicyPopulation.from_policies(members)
    assert len(pop) == P and pop.hidden == hidden and pop.obs_dim == obs_dim and pop.n_out == n_out and pop.out == "tanh"
    fan_in = hidden if hidden else obs_dim
    assert tuple(pop.w2.shape) == (P, n_out, fan_in) and tuple(pop.b2.shape) == (P, n_out)
    if hidden:
        assert tuple(pop.w1.shape) == (P, hidden, obs_dim) and tuple(pop.b1.shape) == (P, hidden)
    else:
        assert pop.w1 is None and pop.b1 is None
    st = pop.struct()
    assert (st.struct_size, st.hidden, st.out_mode, st.reserved) == (C.sizeof(_lib.EmeiPolicy), hidden, _lib.POLICY_OUT_TANH, 0)
    sizes = dict(w1=hidden * obs_dim, b1=hidden, w2=n_out * fan_in, b2=n_out)  # floats per member: the offsets of the header
    for k in ("w1", "b1", "w2", "b2"):
        t = getattr(pop, k)
        if t is None:
            assert getattr(st, k) in (None, 0)
            continue
        assert t.dtype == torch.float32 and t.is_contiguous() and getattr(st, k) == t.data_ptr()
        flat = np.ctypeslib.as_array(C.cast(getattr(st, k), C.POINTER(C.c_float)), shape=(P * sizes[k],))
        for p in range(P):
            m = pop[p]
            assert isinstance(m, MLPPolicy) and m.out == "tanh" and m.hidden == hidden
            assert getattr(m, k).data_ptr() == t.data_ptr() + 4 * p * sizes[k]  # a view of member p, at the documented offset
            assert torch.equal(getattr(m, k), getattr(members[p], k))  # the round trip
            assert np.array_equal(flat[p * sizes[k]:(p + 1) * sizes[k]], getattr(members[p], k).numpy().reshape(-1))
    assert torch.equal(pop[-1].w2, members[-1].w2)
    with pytest.raises(IndexError):
        pop[P]
    # the constructor takes the stacked tensors as they are (other dtypes and layouts are converted)
    again = PolicyPopulation(pop.w2.double().transpose(1, 2).contiguous().transpose(1, 2), pop.b2, pop.w1, pop.b1, out="tanh")
    assert again.w2.dtype == torch.float32 and again.w2.is_contiguous() and torch.equal(again.w2, pop.w2)


def test_shape_and_out_mismatches_raise():
    from emei_amd.policy import PolicyPopulation

    a, b = _members(2, 4, 5, 1)
    with pytest.raises(ValueError, match="out"):
        PolicyPopulation.from_policies([a, _members(1, 4, 5, 1, out="tanh")[0]])
    with pytest.raises(ValueError, match="w1"):
        PolicyPopulation.from_policies([a, _members(1, 4, 0, 1)[0]])  # affine among hidden-layer members
    with pytest.raises(ValueError, match=r"w1 \(6, 4\)"):
        PolicyPopulation.from_policies([a, _members(1, 4, 6, 1)[0]])
    with pytest.raises(ValueError, match="w2"):
        PolicyPopulation.from_policies([_members(1, 4, 0, 1)[0], _members(1, 5, 0, 1)[0]])
    with pytest.raises(ValueError, match="non-empty"):
        PolicyPopulation.from_policies([])
    with pytest.raises(ValueError, match="MLPPolicy"):
        PolicyPopulation.from_policies([a, "b"])
    z = torch.zeros
    with pytest.raises(ValueError, match="out"):
        PolicyPopulation(z(2, 1, 4), z(2, 1), out="softmax")
    with pytest.raises(ValueError, match="w1 and b1"):
        PolicyPopulation(z(2, 1, 5), z(2, 1), w1=z(2, 5, 4))
    for kw, word in ((dict(w2=z(1, 4), b2=z(1)), "w2"), (dict(w2=z(0, 1, 4), b2=z(0, 1)), "w2"), (dict(w2=z(2, 1, 4), b2=z(2)), "b2"),
                     (dict(w2=z(2, 1, 4), b2=z(3, 1)), "b2"), (dict(w2=z(2, 1, 5), b2=z(2, 1), w1=z(3, 5, 4), b1=z(3, 5)), "w1"),
                     (dict(w2=z(2, 1, 5), b2=z(2, 1), w1=z(5, 4), b1=z(2, 5)), "w1"),
                     (dict(w2=z(2, 1, 5), b2=z(2, 1), w1=z(2, 5, 4), b1=z(2, 6)), "b1"),
                     (dict(w2=z(2, 1, 6), b2=z(2, 1), w1=z(2, 5, 4), b1=z(2, 5)), "w2"),
                     (dict(w2=z(2, 1, 1025), b2=z(2, 1), w1=z(2, 1025, 4), b1=z(2, 1025)), "hidden")):
        with pytest.raises(ValueError, match=word):
            PolicyPopulation(**kw)


def test_bind_checks_the_env_shapes():
    from emei_amd.policy import PolicyPopulation

    class Eng:  # what bind reads of an Engine
        act_dim, obs_dim, env_name, device = 6, 18, "HalfCheetahRunning", torch.device("cpu")

    pop = PolicyPopulation.from_policies(_members(2, 18, 3, 6))
    assert pop.bind(Eng) is pop and pop[1].lo == -1.0 and pop[1].discrete is False
    for members in (_members(2, 17, 3, 6), _members(2, 18, 3, 5)):
        with pytest.raises(ValueError, match="HalfCheetahRunning"):
            PolicyPopulation.from_policies(members).bind(Eng)
