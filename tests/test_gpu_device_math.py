"""The device math primitives of emei_amd/csrc/emei_device.h / emei_math.h, run on the GPU on their own (tests/device/math_probe.hip:
one elementwise kernel per primitive, thread i = element i = lane i % 64) against exact references (tests/device_math_reference.py:
mpmath / long double for float64, NumPy float64 for float32 and Box-Muller).  The env parity tests see these primitives only
through a substep that multiplies a trig error by dt; here every stated bound is asserted directly, no point excluded.

Measured maxima (MI355X, ROCm 7.2.0; every test prints its figures as `MEASURED <op> <value>` before it asserts):

| op, domain                                                        | measured maximum        | asserted            |
|-------------------------------------------------------------------|-------------------------|---------------------|
| two-phase table sincos / sincos_ctx, f64, |x| <= 1e6 (sin, cos)   | 1.504e-16, 1.481e-16    | 2.0e-16             |
| sincos_r, f64, |x| <= 1e6 (sin, cos)                              | 1.147e-16, 1.214e-16    | 2.0e-16             |
| fast_sincosf paths (all three), f32, |x| <= 3e4 (sin, cos)        | 6.083e-8, 6.248e-8      | 1.0e-7              |
| trig_reduce_large, 1e6 < |x| <= DBL_MAX: |r|, residual mod 2 pi   | 3.925, 7.393e-16        | 4, 1e-15            |
| two-phase / sincos_ctx, f64, 1e6 < |x| <= DBL_MAX (sin, cos)      | 6.660e-16, 4.812e-16    | 1.2e-15             |
| sincos_r, f64, |x| > 1e6 (device library sincos)                  | 8.115e-17               | 1.22e-16 (1.5 x)    |
| f32 paths, |x| > 3e4 (device library sincosf)                     | 5.598e-8                | 8.40e-8 (1.5 x)     |
| rotated table / m, upright and hanging InvertedPendulum model     | 2.353e-16               | 5e-16               |
| rcp_r, rcp1_r, div_r f64 (relative)                               | 1.110e-16, 2.125e-15, 2.054e-16 | 2.3e-16, 2.2e-15, 4.5e-16 |
| rsqrt_r f64, 1e-20 <= x <= 1e6 (relative)                         | 1.343e-16               | 2.02e-16 (1.5 x)    |
| rcp_r = rcp1_r = div_r f32; rsqrt_r f32 (relative)                | 5.943e-8; 8.925e-8      | 2^-24; 2^-23        |
| boxmuller: a sweep at 4 angles; b sweep at the largest radius     | 6.305e-7; 1.081e-6      | 1.6e-6              |
| wrap_pi, u01, philox4x32_10, lane independence                    | bit for bit             | bit for bit         |

Every stated bound held as stated; no comment had to be widened.  Mutation checks made while this file was written (local
edits, never committed; the probe rebuilt; the named test run): H2 = 0 in sincos_begin_ctx -> test_sincos_f64_in_range[two_phase]
fails with 3.9e-11; the second Newton step of refine_rcp dropped -> test_reciprocals_f64 fails with 2.1e-15; begin(red) instead of
begin(cold ? red : x_any) -> test_cold_lanes_do_not_change_their_wave_mates_sincos[two_phase-f64] fails in the first layout.
"""
import ctypes as C
import os

import numpy as np
import pytest

import device_math_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "device", "libemei_math_probe.so")

# bounds the project states (emei_math.h, emei_device.h, tests/test_math_accuracy.py)
TABLE_BOUND = 2.0e-16  # table sincos and the polynomial sincos, float64, |x| <= 1e6: absolute
F32_BOUND = 1.0e-7  # fast_sincosf, |x| <= 3e4
REDUCE_BOUND = 1.0e-15  # trig_reduce_large: r = x (mod 2 pi) within
TABLE_LARGE_BOUND = 1.2e-15  # table path behind the reduction
ROTATED_BOUND = 5.0e-16  # times m: three more roundings per table entry
RCP_BOUND, RCP1_BOUND, DIV_BOUND = 2.3e-16, 2.2e-15, 4.5e-16  # relative
BOXMULLER_BOUND = 1.6e-6  # 4.9e-7 (radius) + 5.77 (1.3e-7 + 6e-8)
# no claim in the project: 1.5 x the maximum measured on the MI355X, below the cap that still catches a real defect
LIB_F64_BEYOND_CAP, LIB_F32_BEYOND_CAP, RSQRT_CAP = 1.0e-15, 2.0e-7, 1.0e-15
LIB_F64_BEYOND_BOUND = 1.5 * 8.115e-17  # sincos_r float64, |x| > 1e6
LIB_F32_BEYOND_BOUND = 1.5 * 5.598e-8  # the float32 paths, |x| > 3e4
RSQRT_BOUND = 1.5 * 1.343e-16  # rsqrt_r float64; a lost Newton step leaves ~3e-15
# float32 reciprocals are the compiler's correctly rounded division / square root (hipcc's default): half an ulp, 2^-24 relative,
# per operation — one for 1 / d and n / d, two for 1 / sqrtf(x) (the second applied to a value already off by 2^-24)
F32_DIV_BOUND, F32_RSQRT_BOUND = 2.0 ** -24 * (1 + 1e-6), 2.0 ** -23 * (1 + 1e-6)


def _note(op, value):
    print(f"MEASURED {op} {value:.3e}")


class Probe:
    def __init__(self):
        if not os.path.exists(PROBE):
            raise RuntimeError(f'{PROBE} is missing: build it with python -c "import __graft_entry__ as g; g.build()"')
        self.lib = C.CDLL(PROBE)
        assert self.lib.emei_probe_abi_version() == 1
        self.table = torch.from_numpy(np.array(R.trig_table())).cuda()

    def call(self, name, *args):
        fn = getattr(self.lib, "emei_probe_" + name)
        fn.restype = C.c_int
        conv = []
        for a in args:
            if isinstance(a, torch.Tensor):
                assert a.is_cuda and a.is_contiguous()
                conv.append(C.c_void_p(a.data_ptr()))
            elif isinstance(a, float):
                conv.append(C.c_double(a))
            else:
                conv.append(a)
        rc = fn(*conv, C.c_void_p(0))  # the null stream, which is torch's current stream here
        assert rc == 0, f"{name}: hip error {rc}"
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def probe():
    return Probe()  # a missing library is an ERROR of every test here, never a skip


_SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype in _SIGNED:  # torch has no arithmetic on unsigned words; the kernels only see the bits
        a = a.view(_SIGNED[a.dtype])
    return torch.from_numpy(np.array(a)).cuda()


def _out(like, fill=7.0):
    return torch.full_like(like, fill)


def _suffix(x):
    return {np.dtype(np.float64): "f64", np.dtype(np.float32): "f32"}[x.dtype]


def run_sincos(probe, op, x, rot=(1.0, 0.0)):
    """op: two_phase | ctx | r  ->  s, c as NumPy arrays of x's dtype"""
    xd = _dev(x)
    s, c = _out(xd), _out(xd)
    if op == "r":
        probe.call(f"sincos_r_{_suffix(x)}", xd, s, c, C.c_int64(x.size))
    else:
        probe.call(f"sincos_{op}_{_suffix(x)}", probe.table, float(rot[0]), float(rot[1]), xd, s, c, C.c_int64(x.size))
    return s.cpu().numpy(), c.cpu().numpy()


def run_unary(probe, name, x, n_out):
    xd = _dev(x)
    outs = [_out(xd) for _ in range(n_out)]
    probe.call(f"{name}_{_suffix(x)}", xd, *outs, C.c_int64(x.size))
    return [o.cpu().numpy() for o in outs]


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    """bit for bit; any NaN equals any NaN (the payload of an arithmetic NaN is not part of any contract here)"""
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------------------
# trigonometry
@pytest.mark.parametrize("op", ["two_phase", "ctx", "r"])
def test_sincos_f64_in_range(probe, op):
    """|x| <= 1e6: the table path (two-phase asm LDS read, magic-number rounding; sincos_ctx) and the polynomial sincos_r against
    mpmath / long double — random points of every decade, zeros and denormals, the limit, the ties of the table index, the
    multiples of pi/2."""
    case = R.trig_case("f64_small")
    s, c = run_sincos(probe, op, case["x"])
    es, ec = R.abs_err(s, case["s"]), R.abs_err(c, case["c"])
    _note(f"sincos_{op}_f64 |x|<=1e6 sin", es), _note(f"sincos_{op}_f64 |x|<=1e6 cos", ec)
    assert es <= TABLE_BOUND and ec <= TABLE_BOUND


@pytest.mark.parametrize("op", ["two_phase", "ctx", "r"])
def test_sincos_f32_in_range(probe, op):
    case = R.trig_case("f32_small")
    s, c = run_sincos(probe, op, case["x"])
    es, ec = R.abs_err(s, case["s"]), R.abs_err(c, case["c"])
    _note(f"sincos_{op}_f32 |x|<=3e4 sin", es), _note(f"sincos_{op}_f32 |x|<=3e4 cos", ec)
    assert es <= F32_BOUND and ec <= F32_BOUND


def test_trig_reduce_large(probe):
    """Every binary exponent 2^20 .. 2^1023, the 2^945 switch, DBL_MAX, the double closest to a multiple of pi/2: the reduced
    angle is within [-4, 4] and congruent to x modulo 2 pi within 1e-15 (mpmath at 1300 bits); NaN for +-inf and NaN."""
    x = R.trig_case("f64_large")["x"]
    r = _reduce(probe, x)
    assert np.all(np.isfinite(r))
    _note("trig_reduce_large max |r|", float(np.abs(r).max()))
    assert np.abs(r).max() <= 4.0
    res = R.reduction_residual(x, r)
    _note("trig_reduce_large residual mod 2pi", float(res.max()))
    assert res.max() <= REDUCE_BOUND
    assert np.array_equal(_bits(_reduce(probe, -x)), _bits(-r))  # odd, bit for bit
    assert np.isnan(_reduce(probe, np.array([np.inf, -np.inf, np.nan]))).all()


def _reduce(probe, x):
    xd = _dev(x)
    r = _out(xd)
    probe.call("trig_reduce_large", xd, r, C.c_int64(x.size))
    return r.cpu().numpy()


@pytest.mark.parametrize("op", ["two_phase", "ctx"])
def test_table_sincos_f64_beyond_the_limit(probe, op):
    """finite |x| > 1e6 through the cold branch: reduction + a second run of the table block"""
    case = R.trig_case("f64_large")
    s, c = run_sincos(probe, op, case["x"])
    es, ec = R.abs_err(s, case["s"]), R.abs_err(c, case["c"])
    _note(f"sincos_{op}_f64 |x|>1e6 sin", es), _note(f"sincos_{op}_f64 |x|>1e6 cos", ec)
    assert es <= TABLE_LARGE_BOUND and ec <= TABLE_LARGE_BOUND
    s, c = run_sincos(probe, op, np.array([np.inf, -np.inf, np.nan]))
    assert np.isnan(s).all() and np.isnan(c).all()


def test_library_sincos_beyond_the_limit(probe):
    """sincos_r (float64) and every float32 path repair arguments beyond their limit with the device library's sincos / sincosf."""
    case = R.trig_case("f64_large")
    s, c = run_sincos(probe, "r", case["x"])
    e64 = max(R.abs_err(s, case["s"]), R.abs_err(c, case["c"]))
    _note("sincos_r_f64 |x|>1e6", e64)
    case = R.trig_case("f32_large")
    e32 = 0.0
    for op in ("two_phase", "ctx", "r"):
        s, c = run_sincos(probe, op, case["x"])
        e = max(R.abs_err(s, case["s"]), R.abs_err(c, case["c"]))
        _note(f"sincos_{op}_f32 |x|>3e4", e)
        e32 = max(e32, e)
    assert LIB_F64_BEYOND_BOUND <= LIB_F64_BEYOND_CAP and LIB_F32_BEYOND_BOUND <= LIB_F32_BEYOND_CAP
    assert e64 <= LIB_F64_BEYOND_BOUND and e32 <= LIB_F32_BEYOND_BOUND
    for op, dt in (("r", np.float64), ("two_phase", np.float32), ("ctx", np.float32), ("r", np.float32)):
        s, c = run_sincos(probe, op, np.array([np.inf, -np.inf, np.nan], dt))
        assert np.isnan(s).all() and np.isnan(c).all()


def _invpend_rotations():
    """rot_c, rot_s of both InvertedPendulum models (pendulum_envs.h: trig_rot_c / trig_rot_s) rebuilt from the exported model
    constants: mp r cos / sin of the centre-of-mass angle phi0 (upright) and phi0 + pi (the SwingUp variants)"""
    from emei_amd import _lib as L

    buf = (C.c_double * 64)()
    n = L.lib().emei_model_constants(2, C.cast(buf, C.c_void_p), 64)  # the same vector for all four variants
    assert n >= 6, L.lib().emei_last_error()
    k = np.array(buf[:n])  # [gravity, mc, mp, Icom, r, phi0, ...]
    mpr, phi0 = k[2] * k[4], k[5]
    return {"upright": (mpr * np.cos(phi0), mpr * np.sin(phi0)), "hanging": (mpr * np.cos(phi0 + np.pi), mpr * np.sin(phi0 + np.pi))}


@pytest.mark.parametrize("model", ["upright", "hanging"])
@pytest.mark.parametrize("op", ["two_phase", "ctx"])
def test_rotated_premultiplied_table(probe, op, model):
    """stage_trig_table(rot_c, rot_s): the lookup returns m sin(x + off), m cos(x + off) with m, off of the DOUBLES rot_c, rot_s."""
    rc, rs = _invpend_rotations()[model]
    m = float(np.hypot(rc, rs))
    assert 0.1 < m < 10 and rs != 0.0
    case = R.trig_case("f64_small")
    s, c = run_sincos(probe, op, case["x"], rot=(rc, rs))
    want_s = R.LD(rc) * case["s"] + R.LD(rs) * case["c"]  # m sin(x + off) = rot_c sin x + rot_s cos x, in long double
    want_c = R.LD(rc) * case["c"] - R.LD(rs) * case["s"]
    es, ec = R.abs_err(s, want_s) / m, R.abs_err(c, want_c) / m
    _note(f"rotated table {model} {op} sin / m", es), _note(f"rotated table {model} {op} cos / m", ec)
    assert es <= ROTATED_BOUND and ec <= ROTATED_BOUND


@pytest.mark.parametrize("op", ["two_phase", "ctx"])
def test_table_rotation_special_cases(probe, op):
    """(1, 0) is the plain table bit for bit; a power-of-two rot_c scales exactly (the `rot_c != 1` branch); (0, 1) turns the
    table by a quarter: sin -> cos and cos -> -sin of the plain lookup, bit for bit (the same FMAs on swapped entries)."""
    x = R.trig_case("f64_small")["x"][::7]
    s, c = run_sincos(probe, op, x)
    s1, c1 = run_sincos(probe, op, x, rot=(1.0, -0.0))
    assert np.array_equal(_bits(s), _bits(s1)) and np.array_equal(_bits(c), _bits(c1))
    s2, c2 = run_sincos(probe, op, x, rot=(0.25, 0.0))
    assert np.array_equal(s2, 0.25 * s) and np.array_equal(c2, 0.25 * c)
    s3, c3 = run_sincos(probe, op, x, rot=(0.0, 1.0))
    assert np.array_equal(s3, c) and np.array_equal(c3, -s)
    # the plain table agrees with sincos_ctx / the two-phase form of each other
    so, co = run_sincos(probe, "ctx" if op == "two_phase" else "two_phase", x)
    assert R.abs_err(so, s) <= 2 * TABLE_BOUND and R.abs_err(co, c) <= 2 * TABLE_BOUND


# ---------------------------------------------------------------------------------------------------------------------------
# reciprocals
def test_reciprocals_f64(probe):
    d = R.rcp_inputs()
    rcp, rcp1, _ = run_unary(probe, "recip", d, 3)
    want = R.LD(1) / d.astype(R.LD)
    e, e1 = R.rel_err(rcp, want), R.rel_err(rcp1, want)
    _note("rcp_r f64 rel", e), _note("rcp1_r f64 rel", e1)
    assert e <= RCP_BOUND and e1 <= RCP1_BOUND
    num, den = R.div_inputs()
    nd, dd = _dev(num), _dev(den)
    q = _out(nd)
    probe.call("div_f64", nd, dd, q, C.c_int64(num.size))
    eq = R.rel_err(q.cpu().numpy(), num.astype(R.LD) / den.astype(R.LD))
    _note("div_r f64 rel", eq)
    assert eq <= DIV_BOUND
    x = R.rsqrt_inputs()
    _, _, rsq = run_unary(probe, "recip", x, 3)
    er = R.rel_err(rsq, R.LD(1) / np.sqrt(x.astype(R.LD)))
    _note("rsqrt_r f64 rel", er)
    assert RSQRT_BOUND < RSQRT_CAP and er <= RSQRT_BOUND
    # x = 0: the float64 Newton step multiplies 0 by the seed's +inf and returns NaN (emei_device.h says so; the one caller
    # guards the degenerate case)
    _, _, rsq = run_unary(probe, "recip", np.array([0.0]), 3)
    assert np.isnan(rsq[0])


def test_reciprocals_f32(probe):
    d = R.rcp_inputs(np.float32)
    rcp, rcp1, _ = run_unary(probe, "recip", d, 3)
    want = 1.0 / d.astype(np.float64)
    e, e1 = R.rel_err(rcp, want), R.rel_err(rcp1, want)
    _note("rcp_r f32 rel", e), _note("rcp1_r f32 rel", e1)
    assert e <= F32_DIV_BOUND and e1 <= F32_DIV_BOUND
    num, den = R.div_inputs(np.float32)
    nd, dd = _dev(num), _dev(den)
    q = _out(nd)
    probe.call("div_f32", nd, dd, q, C.c_int64(num.size))
    eq = R.rel_err(q.cpu().numpy(), num.astype(np.float64) / den.astype(np.float64))
    _note("div_r f32 rel", eq)
    assert eq <= F32_DIV_BOUND
    x = R.rsqrt_inputs(np.float32)
    _, _, rsq = run_unary(probe, "recip", x, 3)
    er = R.rel_err(rsq, 1.0 / np.sqrt(x.astype(np.float64)))
    _note("rsqrt_r f32 rel", er)
    assert er <= F32_RSQRT_BOUND
    rcp, _, rsq = run_unary(probe, "recip", np.array([0.0], np.float32), 3)
    assert rsq[0] == np.inf and rcp[0] == np.inf  # float32: 1 / sqrtf(0) = +inf


# ---------------------------------------------------------------------------------------------------------------------------
# angle wrap
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_wrap_pi_is_pymod_pos_for_every_input(probe, dtype):
    """"the same bits in every case": in the domain, beyond it up to the format's maximum, +-inf, NaN"""
    theta = R.wrap_inputs_anywhere(dtype)
    w, p = run_unary(probe, "wrap", theta, 2)
    same = _same_bits(w, p)
    assert same.all(), (theta[~same][:5], w[~same][:5], p[~same][:5])
    assert np.isnan(w[~np.isfinite(theta)]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_wrap_pi_is_numpys_floored_modulo_in_its_domain(probe, dtype):
    """|theta| <= 1e15 (float64) / 1e6 (float32): (theta + pi) % (2 pi) - pi of NumPy in the same dtype, bit for bit, and
    inside [-pi, pi)"""
    theta = R.wrap_inputs_in_domain(dtype)
    w, _ = run_unary(probe, "wrap", theta, 2)
    ok = R.same_wrap(w, R.wrap_reference(theta))
    assert ok.all(), (theta[~ok][:5], w[~ok][:5], R.wrap_reference(theta)[~ok][:5])
    pi = dtype(3.141592653589793)
    assert np.all((w >= -pi) & (w < pi)), theta[~((w >= -pi) & (w < pi))][:5]


# ---------------------------------------------------------------------------------------------------------------------------
# random numbers
def _run_boxmuller(probe, a, b):
    z0, z1 = torch.full(a.shape, 7.0, dtype=torch.float32, device="cuda"), torch.full(a.shape, 7.0, dtype=torch.float32, device="cuda")
    probe.call("boxmuller", a, b, z0, z1, C.c_int64(a.numel()))
    return z0, z1


def test_boxmuller_over_every_input(probe):
    """All 2^24 values of the `a` field (u1 = 2^-24 .. 1: radius 5.77 .. 0) at 4 fixed angles, and all 2^24 values of the `b`
    field at the largest radius, against float64 NumPy.  The differences are taken in float64 on the device."""
    fields = torch.arange(R.BM_FIELDS, dtype=torch.int64, device="cuda")
    words = (fields << 8).to(torch.int32)  # wraps to the same 32 bits
    rad = torch.from_numpy(R.boxmuller_radius(np.arange(R.BM_FIELDS))).cuda()
    assert float(rad[-1]) == 0.0 and abs(float(rad[0]) - R.BM_MAX_RADIUS) < 1e-14
    worst = 0.0
    for b_field in R.BM_FIXED_B_FIELDS:
        b = torch.full_like(words, np.array(b_field << 8, np.uint32).view(np.int32).item())
        z0, z1 = _run_boxmuller(probe, words, b)
        cs, sn = R.boxmuller_direction(b_field)
        e = max(float((z0.double() - rad * float(cs)).abs().max()), float((z1.double() - rad * float(sn)).abs().max()))
        _note(f"boxmuller a sweep, b field {b_field:#x}", e)
        assert bool(torch.isfinite(z0).all()) and bool(torch.isfinite(z1).all())
        assert float(z0[-1]) == 0.0 and float(z1[-1]) == 0.0  # u1 = 1: radius 0
        worst = max(worst, e)
    cs, sn = R.boxmuller_direction(np.arange(R.BM_FIELDS))
    z0, z1 = _run_boxmuller(probe, torch.zeros_like(words), words)
    r0 = R.BM_MAX_RADIUS
    e = max(float((z0.double() - r0 * torch.from_numpy(cs).cuda()).abs().max()), float((z1.double() - r0 * torch.from_numpy(sn).cuda()).abs().max()))
    _note("boxmuller b sweep, a field 0", e)
    worst = max(worst, e)
    assert worst <= BOXMULLER_BOUND


def test_boxmuller_ignores_the_low_bits(probe):
    rng = np.random.default_rng(61)
    a = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    a[:4], b[:4] = [0, 0xFF, 0xFFFFFFFF, 0xFFFFFF00], [0xFF, 0, 0xFFFFFF00, 0xFFFFFFFF]
    z = [_run_boxmuller(probe, _dev(x), _dev(y)) for x, y in ((a, b), (a & np.uint32(0xFFFFFF00), b & np.uint32(0xFFFFFF00)),
                                                              (a | np.uint32(0xFF), b | np.uint32(0xFF)))]
    for other in z[1:]:
        assert torch.equal(z[0][0].view(torch.int32), other[0].view(torch.int32)) and torch.equal(z[0][1].view(torch.int32), other[1].view(torch.int32))


def test_u01(probe):
    rng = np.random.default_rng(62)
    r = np.concatenate([np.array([0, 1, 255, 256, 257, 0x7FFFFFFF, 0x80000000, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF], np.uint32),
                        rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)])
    rd = _dev(r)
    out = torch.full(rd.shape, 7.0, dtype=torch.float32, device="cuda")
    probe.call("u01", rd, out, C.c_int64(r.size))
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(R.u01_reference(r)))
    assert got.min() == 0.0 and got.max() == np.float32(1 - 2.0 ** -24)


@pytest.mark.parametrize("launcher", ["philox", "philox_keys_in_place"])
def test_philox(probe, launcher):
    """philox4x32_10<false> and <true> (round keys bumped in scalar registers) against oracle.philox: seeds with the high word
    set, env >= 2^32, episode and block 0xFFFFFFFF"""
    env, episode, block = R.philox_cases()
    ed, pd, bd = _dev(env), _dev(episode), _dev(block)
    for seed in R.PHILOX_SEEDS:
        out = torch.zeros(env.size * 4, dtype=torch.int32, device="cuda")
        probe.call(launcher, C.c_uint64(seed), ed, pd, bd, out, C.c_int64(env.size))
        got = out.cpu().numpy().view(np.uint32).reshape(-1, 4)
        assert np.array_equal(got, R.philox_oracle(seed, env, episode, block)), hex(seed)
    # and consecutive envs across the 2^32 carry against the vectorised restatement (pinned to the oracle by the CPU suite)
    n = 1000
    env = np.arange(n, dtype=np.uint64) + np.uint64(0xFFFFFFFF - 500)
    z = np.zeros(n, np.uint32)
    out = torch.zeros(n * 4, dtype=torch.int32, device="cuda")
    probe.call(launcher, C.c_uint64(0x5EED), _dev(env), _dev(z), _dev(z), out, C.c_int64(n))
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(-1, 4), R.philox_numpy(0x5EED, env, z, z))


# ---------------------------------------------------------------------------------------------------------------------------
# lane independence of the wave-uniform cold paths
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("op", ["two_phase", "ctx", "r"])
def test_cold_lanes_do_not_change_their_wave_mates_sincos(probe, op, dtype):
    """The cold branches are entered by the whole wave when ANY lane is out of range and select per lane (the second begin() run
    "repeats the first bit for bit"): in-range values evaluated in all-hot waves, then again next to cold lanes — one cold lane
    at lane 0 / 31 / 63, alternating lanes, all cold but one, a fully cold wave, ragged last blocks — must keep their bits; the
    cold lanes meet their own bounds."""
    hot, cold = R.hot_values(dtype), R.cold_values(dtype)
    base_s, base_c = run_sincos(probe, op, hot)
    if dtype is np.float64:
        ref_s, ref_c = R.sincos_mp(cold)
        cold_bound = TABLE_LARGE_BOUND if op != "r" else LIB_F64_BEYOND_BOUND
        hs, hc = R.sincos_mp(hot)
        assert R.abs_err(base_s, hs) <= TABLE_BOUND and R.abs_err(base_c, hc) <= TABLE_BOUND
    else:
        with np.errstate(invalid="ignore"):
            ref_s, ref_c = np.sin(cold.astype(np.float64)), np.cos(cold.astype(np.float64))
        cold_bound = LIB_F32_BEYOND_BOUND
    for name, mask in R.cold_layouts():
        x = R.mix(hot, cold, mask)
        s, c = run_sincos(probe, op, x)
        n = mask.size
        assert np.array_equal(_bits(s[~mask]), _bits(base_s[:n][~mask])) and np.array_equal(_bits(c[~mask]), _bits(base_c[:n][~mask])), name
        k = int(mask.sum())
        assert R.abs_err(s[mask], np.resize(ref_s, k)) <= cold_bound and R.abs_err(c[mask], np.resize(ref_c, k)) <= cold_bound, name


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_cold_lanes_do_not_change_their_wave_mates_wrap(probe, dtype):
    hot, cold = R.hot_values(dtype), R.wrap_cold_values(dtype)
    base, base_p = run_unary(probe, "wrap", hot, 2)
    assert R.same_wrap(base, R.wrap_reference(hot)).all() and _same_bits(base, base_p).all()
    for name, mask in R.cold_layouts():
        x = R.mix(hot, cold, mask)
        w, p = run_unary(probe, "wrap", x, 2)
        n = mask.size
        assert np.array_equal(_bits(w[~mask]), _bits(base[:n][~mask])), name
        assert _same_bits(w, p).all(), name
        in_domain = mask & (x == cold[-1])  # one ulp below -pi: the wrap point, either representative (same_wrap)
        assert in_domain.any() and R.same_wrap(w[in_domain], R.wrap_reference(x[in_domain])).all(), name
        assert np.isnan(w[mask & ~np.isfinite(x)]).all(), name
