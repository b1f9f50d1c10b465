"""tests/kernel_matrix.py against the build and against the CPU oracle: the enumeration is exactly what the Makefile compiles and
body_dispatch.hip routes, and the start rows it hands tests/test_gpu_kernel_matrix.py do what they promise — from the oracle alone."""
import os
import re

import numpy as np
import pytest

import kernel_matrix as KM
import plan_reference as PR
from conftest import ROOT

CSRC = os.path.join(ROOT, "emei_amd", "csrc")
N, FREQ_RATE = 130, 2  # the layer-1 shape of tests/test_gpu_kernel_matrix.py


def _make_list(name):
    """the words of `name := ...` in the Makefile, continuation lines included"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(rf"^{name}\s*:=\s*(.*)$", text, re.M)
    assert m, name
    return m.group(1).split()


def test_rows_are_exactly_the_compiled_translation_units():
    tus, bodies = _make_list("TUS"), _make_list("BODIES")
    assert len(tus) == 16 and len(bodies) == 24 and len(set(tus)) == 16 and len(set(bodies)) == 24
    compiled = {f"pend_tu_{t}" for t in tus} | {f"body_tu_{b}" for b in bodies}
    assert {r.tu for r in KM.ROWS} == compiled
    # without the RK4 flag: one row per four-state unit, two (RK4 false / true) per body unit
    for tu in compiled:
        flags = sorted(r.rk4 for r in KM.ROWS if r.tu == tu)
        assert flags == ([False, True] if tu.startswith("body_tu_") else [False]), tu
    assert len(KM.ROWS) == 16 + 2 * 24
    # the layer-1 extras are runtime flags of units that have a row already
    assert all(any(r.tu == x.tu and not r.rk4 for r in KM.ROWS) for x in KM.EXTRA_ROWS)


def test_body_rows_follow_the_dispatch():
    """the `case` list of body_dispatch.hip: every unit it can return is a row of that env id, solver and precision"""
    text = open(os.path.join(CSRC, "body_dispatch.hip")).read()
    body = text[text.index("switch (L.env_id)"):]
    cases = re.split(r"case\s+(EMEI_\w+)\s*:", body)[1:]
    routed = {}
    for enum, block in zip(cases[0::2], cases[1::2]):
        routed[enum] = set(re.findall(r"body_tu_\w+", block.split("default:")[0]))
    assert set().union(*routed.values()) == {f"body_tu_{b}" for b in _make_list("BODIES")}
    for r in KM.ROWS:
        if r.body:
            assert r.tu in routed[KM.ENUM[r.env]], r
            assert r.tu.endswith("f32") == (r.kw["precision"] == "f32") and ("s_f" in r.tu) == (r.kw.get("solver") == "sweep1"), r
    assert {KM.ENUM[r.env] for r in KM.ROWS if r.body} == set(routed)


def test_matrix_size():
    assert len(KM.ENTRY_POINTS) == 16 and len(KM.SUPPORTED) + len(KM.REFUSED) == 16 * 64
    # every UNSUPPORTED entry bites, and no pair is refused twice
    for entry, pred, _ in KM.UNSUPPORTED:
        assert entry in KM.ENTRY_POINTS and any(pred(r) for r in KM.ROWS), entry
    for e, r in KM.REFUSED:
        assert sum(1 for entry, pred, _ in KM.UNSUPPORTED if entry == e and pred(r)) == 1, (e, r)
    print(f"{len(KM.ROWS)} rows x {len(KM.ENTRY_POINTS)} entry points: {len(KM.SUPPORTED)} supported pairs, {len(KM.REFUSED)} refused")


def _check(row, seed):
    """the promises of row.states(N, seed) / row.actions(N, seed), from the oracle alone"""
    s0, act = row.states(N, seed), row.actions(N, seed)
    st, obs, rew, term = row.oracle_step(s0, act, FREQ_RATE)
    assert s0.shape[0] == N and np.isfinite(s0).all()
    assert np.isfinite(st).all() and np.isfinite(obs).all() and np.isfinite(rew).all()
    active = row.constraint_active(s0)
    if active is not None:
        assert 0.05 <= active.mean() and not active.all(), active.mean()  # constrained rows and free ones side by side
    if row.family in ("ip_staged", "ip"):
        stop = np.abs(np.abs(s0[:, 1]) - np.pi / 2) < 0.2
        assert stop.sum() >= N // 10  # at the hinge stop of +-90 degrees (a row of the Balancing variants only)
    if row.family == "cheetah":
        from oracle import oracle as O

        mask = O.planar_row_mask("cheetah", s0)
        assert ((mask & 0x3F) != 0).sum() >= 5 and ((mask >> 6) != 0).sum() >= 5  # joint limits, floor contact
    if row.family == "hopper":
        from oracle import oracle as O

        mask = O.planar_row_mask("hopper", s0)
        assert ((mask & 7) != 0).sum() >= 5 and (((mask >> 3) & 0xFF) != 0).sum() >= 5 and (((mask >> 11) & 7) != 0).sum() >= 5
    if row.env in KM.TERMINATING:
        assert term.any() and not term.all()
    else:
        assert not term.any()
    skip = PR.undecidable(row.env, obs[None], np.ones(N, np.int32), row.kw)
    assert skip.mean() <= 0.01, f"{int(skip.sum())} of {N} terminal flags are undecidable: choose another seed in kernel_matrix.SEEDS"
    if row.kw["precision"] == "f32":
        tol, floor, _ = row.f32_bound()
        # the float32 mode's observation tolerance is 10 to 200 times the project's 1e-5, and so is the band around a threshold in
        # which its terminal flag is undecidable: at most 2 % of the rows
        skip32 = PR.undecidable(row.env, obs[None], np.ones(N, np.int32), row.kw, tol=tol, floor=floor)
        assert skip32.mean() <= 0.02, int(skip32.sum())
        if row.family == "hopper":
            covered = row.f32_rows(N)
            assert covered[N - N // 4:].all() and covered.sum() >= 0.65 * N  # every capsule-pair row, the ragged wave included
            bad = row.ill_conditioned(s0, act, FREQ_RATE, tol, floor) & covered
            assert bad.mean() <= 0.01, f"{np.nonzero(bad)[0]} are ill-conditioned: choose another seed in kernel_matrix.SEEDS"


@pytest.mark.parametrize("row", KM.LAYER1_ROWS, ids=lambda r: r.id)
def test_start_rows_keep_their_promises(row):
    _check(row, row.seed)
