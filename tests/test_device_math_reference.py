"""tests/device_math_reference.py pinned on the CPU: the input builders really contain the cases the GPU tests
(tests/test_gpu_device_math.py) rely on, the two high-precision references agree, the correctly rounded table is the table
abi.hip builds, the probe library exports its launchers, and the Philox expectation equals the oracle's."""
import os
import subprocess

import mpmath
import numpy as np
import pytest

import device_math_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "device", "libemei_math_probe.so")
LAUNCHERS = ("emei_probe_abi_version", "emei_probe_sincos_two_phase_f64", "emei_probe_sincos_two_phase_f32", "emei_probe_sincos_ctx_f64",
             "emei_probe_sincos_ctx_f32", "emei_probe_sincos_r_f64", "emei_probe_sincos_r_f32", "emei_probe_trig_reduce_large",
             "emei_probe_recip_f64", "emei_probe_recip_f32", "emei_probe_div_f64", "emei_probe_div_f32", "emei_probe_wrap_f64",
             "emei_probe_wrap_f32", "emei_probe_boxmuller", "emei_probe_u01", "emei_probe_philox", "emei_probe_philox_keys_in_place")


def _has(x, v):
    v = np.asarray(v, x.dtype)
    return bool(np.any((x == v) & (np.signbit(x) == np.signbit(v))))


def test_builders_are_deterministic():
    for build in (R.trig_inputs_large_f64, R.trig_inputs_small_f32, R.trig_inputs_large_f32, R.rcp_inputs, R.rsqrt_inputs, R.tie_points,
                  R.half_pi_points, R.hot_values, R.cold_values, R.wrap_inputs_anywhere):
        a, b = build(), build()
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), build.__name__
    (x0, e0), (x1, e1) = R.trig_inputs_small_f64(), R.trig_inputs_small_f64()
    assert np.array_equal(x0, x1) and np.array_equal(e0, e1)
    assert all(np.array_equal(a, b) for a, b in zip(R.philox_cases(), R.philox_cases()))


def test_small_trig_inputs_contain_the_hard_cases():
    x, exact = R.trig_inputs_small_f64()
    assert x.dtype == np.float64 and np.all(np.abs(x) <= R.F64_LIMIT)
    assert 5000 <= exact.sum() <= 50000 and x.size <= 60000
    for v in (0.0, -0.0, 5e-324, -5e-324, 1e-310, 1e6, -1e6, np.nextafter(1e6, 0), -np.nextafter(1e6, 0)):
        assert _has(x[exact], v), v
    mag = np.abs(x[~exact])
    for e in range(-3, 6):  # random points of every decade 1e-3 .. 1e6
        assert ((mag >= 10.0 ** e) & (mag < 10.0 ** (e + 1))).sum() >= 3900, e
    # ties of the table index: x * 256 / (2 pi) within 1e-9 of a half-integer, for every residue k mod 256 and up to |x| ~ 1e6
    ties = R.tie_points()
    n = ties.astype(R.LD) * R.LD(R.TABLE_SIZE) / (2 * R.PI_LD)
    frac = np.abs(n - np.floor(n) - R.LD(0.5)).astype(np.float64)
    assert ties.size == (256 + 4 * 64) * 7 * 2 and frac.max() < 2e-8  # 3.5 ulp of 1e6 times 256 / (2 pi)
    assert len(set((np.floor(n[ties > 0]).astype(np.int64) % 256).tolist())) == 256 and np.abs(ties).max() > 9.9e5
    assert np.all(np.isin(ties, x[exact]))
    # multiples of pi/2: both sides of the exact multiple are present
    hp = R.half_pi_points()
    q = hp.astype(R.LD) / (R.PI_LD / 2)
    assert np.abs(q - np.rint(q)).max() < 1e-9 and (q > np.rint(q)).sum() > 100 and (q < np.rint(q)).sum() > 100
    assert np.all(np.isin(hp, x[exact])) and np.abs(hp).max() > 9.9e5

    f = R.trig_inputs_small_f32()
    assert f.dtype == np.float32 and np.all(np.abs(f) <= R.F32_LIMIT)
    for v in (0.0, -0.0, 1e-45, 3e4, -3e4, np.nextafter(np.float32(3e4), np.float32(0))):
        assert _has(f, np.float32(v)), v


def test_large_trig_inputs_contain_the_hard_cases():
    x = R.trig_inputs_large_f64()
    assert x.dtype == np.float64 and np.all(np.isfinite(x)) and np.all(np.abs(x) > R.F64_LIMIT) and x.size <= 50000
    assert np.array_equal(np.sort(x), np.sort(-x))  # negative copies of all of them
    _, e = np.frexp(x[x > 0])
    counts = np.bincount(e - 1, minlength=1024)  # frexp: x = m 2^e with m in [0.5, 1)
    assert np.all(counts[20:1024] >= 8) and counts[:19].sum() == 0
    for v in (2.0 ** 945, np.nextafter(2.0 ** 945, 0), np.nextafter(2.0 ** 945, np.inf), R.DBL_MAX, 6381956970095103.0 * 2.0 ** 797,
              np.nextafter(1e6, np.inf), 2.0 ** 20, 2.0 ** 1023):
        assert _has(x, v) and _has(x, -v), v

    f = R.trig_inputs_large_f32()
    assert f.dtype == np.float32 and np.all(np.isfinite(f)) and np.all(np.abs(f) > R.F32_LIMIT)
    _, e = np.frexp(f[f > 0])
    assert np.all(np.bincount(e - 1, minlength=128)[15:128] >= 8)
    assert _has(f, R.FLT_MAX) and _has(f, -R.FLT_MAX) and _has(f, np.nextafter(np.float32(3e4), np.float32(np.inf)))


def test_cold_lane_layouts():
    layouts = R.cold_layouts()
    assert len(layouts) == 1 + 2 * len(R.RAGGED_TAILS) == 7
    assert sorted({m.size % 256 for _, m in layouts}) == [0, 1, 63, 65]
    full = layouts[0][1].reshape(-1, R.WAVE)
    assert full.shape == (8, 64)
    assert [int(w.sum()) for w in full] == [1, 1, 1, 32, 32, 63, 64, 0]
    assert full[0, 0] and full[1, 31] and full[2, 63] and not full[5, 17]
    assert np.array_equal(full[3], ~full[4])
    for name, m in layouts[1:]:
        assert np.array_equal(m[:512], layouts[0][1]) and m[512] == ("cold_first" in name)
    for dt in (np.float64, np.float32):
        hot, cold = R.hot_values(dt), R.cold_values(dt)
        lim = R.F64_LIMIT if dt is np.float64 else R.F32_LIMIT
        assert hot.dtype == dt and hot.size == R.LAYOUT_MAX_N == 577 and np.all(np.abs(hot) <= lim) and _has(hot, lim)
        assert cold.dtype == dt and np.all(~(np.abs(cold) <= lim)) and np.isnan(cold).sum() == 1 and np.isinf(cold).sum() == 2
        x = R.mix(hot, cold, layouts[-1][1])
        assert np.array_equal(x[~layouts[-1][1]], hot[~layouts[-1][1]]) and np.all(~(np.abs(x[layouts[-1][1]]) <= lim))
        w = R.wrap_cold_values(dt)
        assert w.dtype == dt and np.isnan(w).sum() == 1 and np.isinf(w).sum() == 2 and w[-1] < dt(-np.pi)


def test_reciprocal_and_wrap_inputs():
    d = R.rcp_inputs()
    assert np.abs(d).min() == 2.0 ** -20 and np.abs(d).max() == 2.0 ** 20 and (d < 0).sum() == (d > 0).sum() and d.size <= 100000
    assert ((np.abs(d) > 0.05) & (np.abs(d) < 20)).sum() >= 40000
    n, d2 = R.div_inputs()
    assert np.array_equal(d, d2) and np.abs(n).min() >= 1e-3 and np.abs(n).max() <= 1e3
    x = R.rsqrt_inputs()
    assert x.min() == 1e-20 and x.max() == 1e6
    t = R.wrap_inputs_in_domain()
    assert np.abs(t).max() == 1e15 and _has(t, np.pi) and _has(t, -np.pi) and _has(t, np.nextafter(-np.pi, -np.inf))
    mag = np.abs(t)
    for e in range(-3, 15):
        assert ((mag >= 10.0 ** e) & (mag < 10.0 ** (e + 1))).sum() >= 2400, e
    assert np.abs(R.wrap_inputs_in_domain(np.float32)).max() == 1e6
    for dt in (np.float64, np.float32):
        a = R.wrap_inputs_anywhere(dt)
        assert a.dtype == dt and np.isnan(a).sum() == 1 and np.isinf(a).sum() == 2 and _has(a, np.finfo(dt).max)
    # the reference itself: inside [-pi, pi] and congruent to theta
    ref = R.wrap_reference(t)
    assert np.all(np.abs(ref) <= np.pi)
    small = np.abs(t) < 1e3
    assert np.abs(np.angle(np.exp(1j * (ref[small] - t[small])))).max() < 1e-12


def test_mpmath_and_longdouble_references_agree():
    assert np.finfo(R.LD).eps < 1.2e-19  # x87 extended: the long-double reference is worth its name
    x, exact = R.trig_inputs_small_f64()
    sample = np.concatenate([x[exact][::23], x[~exact][::61]])
    s_mp, c_mp = R.sincos_mp(sample)
    s_ld, c_ld = R.sincos_ld(sample)
    assert np.abs(s_mp - s_ld).max() <= 1e-18 and np.abs(c_mp - c_ld).max() <= 1e-18
    # mpmath's own huge-argument reduction against an independent 3000-bit evaluation
    for v in (R.DBL_MAX, R.CLOSEST_TO_HALF_PI_MULTIPLE, -1e300):
        s, c = R.sincos_mp(np.array([v]))
        with mpmath.workprec(3000):
            r = mpmath.mpf(v) - mpmath.nint(mpmath.mpf(v) / (2 * mpmath.pi)) * 2 * mpmath.pi
            assert abs(mpmath.sin(r) - mpmath.mpf(float(s[0]))) < 1e-15 and abs(mpmath.cos(r) - mpmath.mpf(float(c[0]))) < 1e-15
    assert abs(float(R.sincos_mp(np.array([R.CLOSEST_TO_HALF_PI_MULTIPLE]))[1][0])) < 1e-18  # cos: 4.7e-19 away from a zero
    s, c = R.sincos_mp(np.array([np.inf, -np.inf, np.nan]))
    assert np.isnan(s).all() and np.isnan(c).all()
    assert R.reduction_residual(np.array([1e300, 7.0]), np.array([1e300, 7.0 - 2 * np.pi])).max() < 1e-15
    assert abs(R.reduction_residual(np.array([10.0]), np.array([10.0 - 4 * np.pi + 0.25]))[0] - 0.25) < 1e-14  # it does see a miss


def test_correctly_rounded_table_is_the_table_of_the_abi():
    """(double)sinl / cosl of 2 pi_l k / 256 (abi.hip:emei_trig_table) IS the correctly rounded table — except at the three exact
    zeros (cos at k = 64 and 192, sin at k = 128), where the long-double pi leaves sin / cos of its own rounding error, at most
    1.9e-19, in place of 0: three orders of magnitude below every bound of the table path."""
    tab, host = R.trig_table(), R.trig_table_host_formula()
    assert tab.shape == host.shape == (256, 2)
    zeros = np.zeros((256, 2), bool)
    zeros[64, 1] = zeros[128, 0] = zeros[192, 1] = True
    assert np.array_equal(tab[~zeros], host[~zeros])
    assert np.all(tab[zeros] == 0.0) and np.abs(host[zeros]).max() <= 1.9e-19
    assert tab[0].tolist() == [0.0, 1.0] and tab[64].tolist() == [1.0, 0.0] and tab[128].tolist() == [0.0, -1.0] and tab[192].tolist() == [-1.0, 0.0]
    assert np.abs(np.hypot(tab[:, 0], tab[:, 1]) - 1).max() <= 2.3e-16


def test_probe_library_exports_its_launchers():
    assert os.path.exists(PROBE), 'no probe library: run python -c "import __graft_entry__ as g; g.build()"'
    out = subprocess.run(["nm", "-D", "--defined-only", PROBE], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(LAUNCHERS) <= exported, sorted(set(LAUNCHERS) - exported)
    assert not any(s.startswith("emei_") and not s.startswith("emei_probe_") for s in exported)  # none of the product's ABI


def test_philox_expectation_is_the_oracles():
    env, episode, block = R.philox_cases()
    assert env.dtype == np.uint64 and int(env.max()) == 2 ** 64 - 1 and (env >= 2 ** 32).sum() > 300
    assert (episode == 0xFFFFFFFF).any() and (block == 0xFFFFFFFF).any() and ((episode == 0xFFFFFFFF) & (block == 0xFFFFFFFF)).any()
    assert any(s >> 32 for s in R.PHILOX_SEEDS) and 0 in R.PHILOX_SEEDS
    for seed in R.PHILOX_SEEDS:
        assert np.array_equal(R.philox_numpy(seed, env, episode, block), R.philox_oracle(seed, env, episode, block)), hex(seed)
    for ctr, key, want in R.PHILOX_KAT:  # the published known answers
        got = R.philox_numpy(key[0] | key[1] << 32, np.array([ctr[0] | ctr[1] << 32], np.uint64), [ctr[2]], [ctr[3]])
        assert got[0].tolist() == list(want)


def test_random_number_references():
    assert R.u01_reference(np.array([0, 255, 256, 0xFFFFFFFF], np.uint32)).tolist() == [0.0, 0.0, 2.0 ** -24, 1 - 2.0 ** -24]
    assert R.boxmuller_radius(R.BM_FIELDS - 1) == 0.0 and R.boxmuller_radius(0) == pytest.approx(R.BM_MAX_RADIUS, rel=1e-15)
    assert R.BM_MAX_RADIUS == pytest.approx(5.768, abs=1e-3)
    c, s = R.boxmuller_direction(np.array([0, R.BM_FIELDS // 4, R.BM_FIELDS // 2]))
    assert np.abs(c - [1, 0, -1]).max() < 2e-16 and np.abs(s - [0, 1, 0]).max() < 2e-16
    assert R.BM_FIXED_B_FIELDS[0] == 0 and R.BM_FIXED_B_FIELDS[-1] == R.BM_FIELDS - 1 and len(R.BM_FIXED_B_FIELDS) == 4
