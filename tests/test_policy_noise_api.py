"""emei_rollout_policy_noisy on the host: declared (additive under ABI 8), exported and bound; the header carries the history line, the
normative comment, the enum, the struct and the kernel ids; every refusal that precedes the handle comes back EMEI_ERR_INVALID with a
message that starts with `emei_rollout_policy_noisy:` and names the argument, for a NULL handle and before any HIP call (no GPU
needed), in the header's order.  And the host logic of PolicyNoise on CPU tensors."""
import ctypes as C
import os
import re
import subprocess

import pytest

from emei_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "emei_rollout_policy_noisy"


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "emei_hip.h")).read()
    proto = re.search(r"EMEI_API\s+int\s+emei_rollout_policy_noisy\s*\(([^;]*)\)\s*;", hdr)
    assert proto
    args = [a.strip() for a in " ".join(proto.group(1).split()).split(",")]
    assert args == ["emei_env* h", "int32_t n_steps", "const emei_policy* policy", "const emei_policy_noise* noise", "void* actions_out",
                    "int action_dtype", "float* obs_out", "float* reward_out", "uint8_t* done_out", "uint32_t flags", "void* stream"]
    assert len(_lib.SYMBOLS[FN][1]) == len(args)
    assert re.search(r"#define\s+EMEI_ABI_VERSION\s+8\b", hdr)  # additive: the version stays
    assert re.search(r"enum\s+emei_policy_noise_mode\s*\{\s*EMEI_POLICY_NOISE_GAUSS\s*=\s*0\s*,[^}]*EMEI_POLICY_NOISE_GAUSS_HEAD\s*=\s*1\s*,[^}]*"
                     r"EMEI_POLICY_NOISE_EPS_GREEDY\s*=\s*2[^}]*\}", hdr)
    assert (_lib.POLICY_NOISE_GAUSS, _lib.POLICY_NOISE_GAUSS_HEAD, _lib.POLICY_NOISE_EPS_GREEDY) == (0, 1, 2)
    for name, val, py in (("EMEI_KERNEL_PEND_POLICY_NOISY", 18, _lib.KERNEL_PEND_POLICY_NOISY),
                          ("EMEI_KERNEL_BODY_POLICY_NOISY", 19, _lib.KERNEL_BODY_POLICY_NOISY),
                          ("EMEI_KERNEL_BODY_POLICY_NOISY_RK4", 20, _lib.KERNEL_BODY_POLICY_NOISY_RK4)):
        assert re.search(name + r"\s*=\s*%d\b" % val, hdr) and py == val and "noisy" in _lib.kernel_name(val), name
    # the older tables keep their ids; one lookup serves all three
    assert sorted(_lib.POLICY_NOISY_KERNEL_NAMES) == [18, 19, 20] and sorted(_lib.POLICY_KERNEL_NAMES) == [15, 16, 17]
    assert len(_lib.KERNEL_NAMES) == 15 and _lib.kernel_name(5) == _lib.KERNEL_NAMES[5] and _lib.kernel_name(16) == _lib.POLICY_KERNEL_NAMES[16]
    # the struct: field for field
    body = hdr[hdr.index("typedef struct emei_policy_noise {"):hdr.index("} emei_policy_noise;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*([\w\s,]+);", body, re.M) for n in decl.split(",")]
    assert fields == ["struct_size", "mode", "seed", "sigma", "std", "ws", "bs", "log_std_min", "log_std_max", "reserved"]
    assert [f[0] for f in _lib.EmeiPolicyNoise._fields_] == fields
    assert _lib.EmeiPolicyNoise.seed.offset == 8 and _lib.EmeiPolicyNoise.sigma.offset == 16 and _lib.EmeiPolicyNoise.std.offset == 24
    # the history line, and a normative comment of its own in front of the enum
    assert FN in hdr[hdr.index("ABI history"):hdr.index("#define EMEI_ABI_VERSION")]
    after = hdr[hdr.index("EMEI_API int emei_rollout_policy("):]
    comment = after[:after.index("enum emei_policy_noise_mode")]
    for word in ("Noise words", "philox4x32_10", "seed + t", "mod 2^64", "candidate k = 0", "harmless", "Box-Muller", "(q & 1) ? z1 : z0",
                 "(double)s_q * (double)z_q", "last", "std[q]", "(float)sigma", "does not fault", "log_std_min", "float64 exp", "NOT pinned",
                 "explore = u(W[0]) < (float)sigma", "u(W[1]) < 0.5f", "Replay", "Chunking", "(b, seed + a)", "Sharding",
                 "neither allocates nor synchronises", "pend_policy_rollout_noisy_kernel", "body_policy_rollout_noisy_kernel", "seed + t + 1",
                 "EMEI_ERR_INVALID", "EMEI_ERR_STATE", "EMEI_ERR_UNSUPPORTED", "DEVICE pointers"):
        assert word in comment, word
    lib = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert FN in _lib.SYMBOLS and FN in exported and hasattr(lib, FN)
    assert lib.emei_abi_version() == 8 and _lib.ABI_VERSION == 8


def _caller():
    lib = _lib.lib()
    buf = {k: C.cast((C.c_double * 64)(), C.c_void_p) for k in ("w1", "b1", "w2", "b2", "std", "ws", "bs", "act", "obs", "rew", "done")}
    psize, nsize = C.sizeof(_lib.EmeiPolicy), C.sizeof(_lib.EmeiPolicyNoise)

    def call(n_steps=3, policy=True, p_size=psize, hidden=4, out_mode=0, p_reserved=0, w2=buf["w2"], noise=True, struct_size=nsize, mode=0,
             seed=7, sigma=0.5, std=None, ws=None, bs=None, lmin=-20.0, lmax=2.0, reserved=0, dtype=_lib.ACT_U8, flags=0):
        pol = _lib.EmeiPolicy(p_size, hidden, out_mode, p_reserved, buf["w1"], buf["b1"], w2, buf["b2"])
        nz = _lib.EmeiPolicyNoise(struct_size, mode, seed, sigma, std, ws, bs, lmin, lmax, reserved)
        rc = lib.emei_rollout_policy_noisy(None, n_steps, C.byref(pol) if policy else None, C.byref(nz) if noise else None, buf["act"], dtype,
                                           buf["obs"], buf["rew"], buf["done"], flags, None)
        return rc, lib.emei_last_error().decode()

    return call, buf, nsize


def test_sizeof_matches_the_binding():
    call, _, nsize = _caller()
    rc, msg = call(struct_size=0)
    assert rc == _lib.ERR_INVALID
    assert int(re.search(r"sizeof\(emei_policy_noise\)=(\d+)", msg).group(1)) == nsize == 64


def test_refusals_with_a_null_handle():
    call, buf, nsize = _caller()
    nan, inf = float("nan"), float("inf")
    G, HEAD, EPS = _lib.POLICY_NOISE_GAUSS, _lib.POLICY_NOISE_GAUSS_HEAD, _lib.POLICY_NOISE_EPS_GREEDY
    head = dict(mode=HEAD, ws=buf["ws"], bs=buf["bs"])
    rc, msg = call()
    assert rc == _lib.ERR_INVALID and msg.startswith(FN + ":") and "null handle" in msg, msg
    cases = (({"n_steps": 0}, "n_steps"), ({"policy": False}, "null policy"), ({"p_size": 8}, "policy.struct_size"),
             ({"hidden": -1}, "policy.hidden"), ({"hidden": 1025}, "policy.hidden"), ({"out_mode": 2}, "policy.out_mode"),
             ({"p_reserved": 1}, "policy.reserved"),
             ({"noise": False}, "null noise"),
             ({"struct_size": 0}, "noise.struct_size"), ({"struct_size": nsize - 8}, "noise.struct_size"), ({"struct_size": nsize + 8}, "noise.struct_size"),
             ({"mode": 3}, "noise.mode"), ({"mode": -1}, "noise.mode"), ({"reserved": 1}, "noise.reserved"), ({"reserved": -7}, "noise.reserved"),
             ({"sigma": -0.5}, "noise.sigma"), ({"sigma": nan}, "noise.sigma"), ({"sigma": inf}, "noise.sigma"), ({"sigma": -inf}, "noise.sigma"),
             ({"mode": EPS, "sigma": -0.01}, "noise.sigma"), ({"mode": EPS, "sigma": 1.0000001}, "noise.sigma"), ({"mode": EPS, "sigma": nan}, "noise.sigma"),
             (dict(head, lmin=2.5), "noise.log_std_min"), (dict(head, lmin=nan), "noise.log_std_min"), (dict(head, lmax=nan), "noise.log_std_m"),
             (dict(head, ws=None), "null noise.ws"), (dict(head, bs=None), "null noise.bs"), (dict(head, ws=None, bs=None), "null noise.ws"))
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and msg.startswith(FN + ":") and word in msg, (kw, rc, msg)
    # the edges pass the checks that need no handle: the handle is what is named
    for kw in ({"sigma": 0.0}, {"sigma": 1e30}, {"mode": EPS, "sigma": 0.0}, {"mode": EPS, "sigma": 1.0}, dict(head, lmin=2.0, lmax=2.0),
               dict(head, lmin=-inf, lmax=inf), {"sigma": nan, "std": buf["std"]},  # a given std: sigma is not consulted
               dict(head, sigma=nan), {"seed": 2 ** 64 - 1}, {"mode": EPS, "std": buf["std"], "sigma": 0.25}):
        assert "null handle" in call(**kw)[1], kw
    # in the order of the header: the policy struct, then the noise struct field by field, then the handle
    bad = {"n_steps": 0, "policy": False, "noise": False}
    for key, word in (("n_steps", "n_steps"), ("policy", "null policy"), ("noise", "null noise")):
        msg = call(**bad)[1]
        assert word in msg and msg.startswith(FN + ":"), (key, msg)
        del bad[key]
    bad = {"p_reserved": 3, "struct_size": 1, "mode": 9, "reserved": 3, "sigma": -1.0}
    for key, word in (("p_reserved", "policy.reserved"), ("struct_size", "noise.struct_size"), ("mode", "noise.mode"), ("reserved", "noise.reserved")):
        msg = call(**bad)[1]
        assert word in msg, (key, msg)
        del bad[key]
    assert "noise.sigma" in call(**bad)[1]
    bad = dict(mode=HEAD, reserved=2, lmin=3.0, ws=None, bs=None)
    for key, word in (("reserved", "noise.reserved"), ("lmin", "noise.log_std_min"), ("ws", "null noise.ws"), ("bs", "null noise.bs")):
        msg = call(**bad)[1]
        assert word in msg, (key, msg)
        if key in ("ws", "bs"):
            bad[key] = buf[key]
        else:
            del bad[key]
    assert "null handle" in call(**bad)[1]
    # what comes after the handle (the weights, the dtype, the flags, the mode against the env kind) does not win over it
    assert "null handle" in call(w2=None, dtype=77, flags=0xF0)[1]
    assert "noise.reserved" in call(reserved=1, w2=None, dtype=77, flags=0xF0)[1]
    with pytest.raises(ValueError, match="noise.mode"):
        _lib.check(call(mode=5)[0])


def test_the_messages_of_emei_rollout_policy_stay():
    """the two calls share their checks: the messages tests/test_policy_population_api.py quotes are what they were"""
    lib = _lib.lib()
    pol = _lib.EmeiPolicy(C.sizeof(_lib.EmeiPolicy), -1, 0, 0, None, None, None, None)
    assert lib.emei_rollout_policy(None, 3, C.byref(pol), None, 0, None, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.emei_last_error().decode() == "emei_rollout_policy: policy.hidden=-1 is outside [0, EMEI_POLICY_MAX_HIDDEN=1024]"
    assert lib.emei_rollout_policy(None, 3, None, None, 0, None, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.emei_last_error().decode() == "emei_rollout_policy: null policy"
    assert lib.emei_rollout_policy_noisy(None, 3, None, None, None, 0, None, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.emei_last_error().decode() == "emei_rollout_policy_noisy: null policy"


# ---------------------------------------------------------------------------------------------- PolicyNoise, on CPU tensors
torch = pytest.importorskip("torch")


def test_policy_noise_host_logic():
    import emei_amd
    from emei_amd.policy import PolicyNoise

    assert emei_amd.PolicyNoise is PolicyNoise
    for kw in ({}, dict(std=0.1, epsilon=0.1), dict(std=0.1, log_std_head=([[0.0]], [0.0])), dict(std=0.1, epsilon=0.2, log_std_head=([[0.0]], [0.0]))):
        with pytest.raises(ValueError, match="exactly one"):
            PolicyNoise(1, **kw)
    for kw, word in ((dict(epsilon=1.5), "epsilon"), (dict(epsilon=float("nan")), "epsilon"), (dict(std=-1.0), "std"), (dict(std=float("inf")), "std"),
                     (dict(std=[[0.1]]), "std"), (dict(log_std_head=([0.0], [0.0])), "log_std_head"),
                     (dict(log_std_head=([[0.0]], [0.0]), log_std_range=(1.0, -1.0)), "log_std_range")):
        with pytest.raises(ValueError, match=word):
            PolicyNoise(1, **kw)
    s = PolicyNoise(2 ** 64 + 5, std=0.25).struct()
    assert (s.struct_size, s.mode, s.seed, s.sigma, s.std, s.ws, s.bs, s.reserved) == (64, _lib.POLICY_NOISE_GAUSS, 5, 0.25, None, None, None, 0)
    n = PolicyNoise(3, std=[0.1, 0.2, 0.3])
    s = n.struct()
    assert s.std == n.std.data_ptr() and n.std.dtype == torch.float32 and s.sigma == 0.0
    s = PolicyNoise(3, epsilon=0.25).struct()
    assert (s.mode, s.sigma) == (_lib.POLICY_NOISE_EPS_GREEDY, 0.25)
    n = PolicyNoise(3, log_std_head=(torch.zeros(3, 5), torch.zeros(3)), log_std_range=(-5.0, 1.0))
    s = n.struct(5)
    assert (s.mode, s.ws, s.bs, s.log_std_min, s.log_std_max) == (_lib.POLICY_NOISE_GAUSS_HEAD, n.ws.data_ptr(), n.bs.data_ptr(), -5.0, 1.0)
    with pytest.raises(ValueError, match="like the policy's w2"):
        n.struct(4)
    # bind: the mode against the env kind, the shapes against the action space
    eng = lambda name, ad: type("E", (), dict(env_name=name, act_dim=ad, device=torch.device("cpu")))()
    with pytest.raises(ValueError, match="discrete"):
        PolicyNoise(1, std=0.1).bind(eng("CartPoleSwingUp", 0))
    with pytest.raises(ValueError, match="continuous"):
        PolicyNoise(1, epsilon=0.1).bind(eng("HopperRunning", 3))
    with pytest.raises(ValueError, match="3 policy output"):
        PolicyNoise(1, std=[0.1, 0.2]).bind(eng("HopperRunning", 3))
    assert PolicyNoise(1, std=[0.1, 0.2, 0.3]).bind(eng("HopperRunning", 3)).bound_engine().act_dim == 3
    with pytest.raises(ValueError, match="bind"):
        PolicyNoise(1, std=0.1).bound_engine()
    # the head's scale on host tensors is the clause: float32(exp(clamp(ws @ h + bs)))
    n = PolicyNoise(1, log_std_head=([[1.0, 0.0], [0.0, -100.0]], [0.5, 0.0]))
    h = torch.tensor([[1.0, 1.0], [100.0, -1.0]], dtype=torch.float64)
    want = torch.exp(torch.tensor([[1.5, -20.0], [2.0, 2.0]], dtype=torch.float64)).to(torch.float32)
    assert torch.equal(n.scale(h), want)
