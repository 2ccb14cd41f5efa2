"""Shape code 7 (CS_SHAPE_VOIGT_LBL: code 6 at pressure-shifted centres, include/clearsky_hip.h) on the host side: the code in every
table that maps shape names, the refusals Python makes before any device call, the restatement the GPU tests build their expected
values from (tests/voigt_lbl_ref.py) against 40-digit arithmetic on one-line slices, and the premises of the device cases, checked on
the reference alone.  No GPU needed.

The reference's own error (test_restatement_vs_40_digits, oracle identity against 40 digits, over the sum before the pedestal comes
off): worst ratio 7.0e-15 on the exact-shift table at cut-offs 1, 5 and 25 (1.4e-14 on the golden file's own shifts), so the
restatement can hold the device to 1e-11; the test asserts 1e-12, a tenth of that bar."""
import inspect
import os
import re

import numpy as np
import pytest

import ckdvvh_ref as X
import lineparam_ref as LP
import voigt_lbl_ref as V
from conftest import HITRAN, ROOT
from test_gpu_pressure_shift import write_par

KATM = V.KATM


def _read(*p):
    with open(os.path.join(ROOT, *p), encoding="utf-8") as f:
        return f.read()


@pytest.fixture(scope="module")
def case(cs, tmp_path_factory):
    """the exact-shift table of the device cases, through a .par file"""
    t = V.case_table()
    path = os.path.join(str(tmp_path_factory.mktemp("lbl")), "case.par")
    sl = cs.SpectralLines(write_par(path, 1, t["nu"], t["S"], t["gamma_a"], t["gamma_s"], t["Epp"], t["na"], t["delta_a"]))
    assert np.array_equal(sl.nu, t["nu"]) and np.array_equal(sl.delta_a, t["delta_a"])
    return sl


def test_names_header_and_julia(cs):
    assert cs.SHAPES["voigtLBL"] == 7
    assert callable(cs.voigtLBL) and callable(cs.voigtLBL_)
    assert inspect.signature(cs.voigtLBL).parameters["dnu_cut"].default == 25.0
    h = _read("include", "clearsky_hip.h")
    enum = re.search(r"enum\s*\{\s*CS_SHAPE_VOIGT\s*=\s*0[^}]*\}", h).group(0)
    assert re.search(r"CS_SHAPE_VOIGT_LBL\s*=\s*7", enum) and re.search(r"CS_SHAPE_VOIGT_CKD_VVH\s*=\s*6", enum)
    src = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", h, flags=re.S))
    protos = set(re.findall(r"\b(?:const\s+)?(?:int|void|char)\s*\**\s*(cs_\w+)\s*\([^;{]*?\)\s*;", src, flags=re.S))
    assert len(protos) == 48, len(protos)
    assert len(cs.SIGNATURES) == 62
    j = _read("julia", "ClearSkyHIP.jl")
    assert re.search(r"const SHAPES = Dict\([^)]*:voigtLBL=>7", j)
    assert "slotfrompar!" in j[j.index(":voigtLBL=>7"):][:600]          # (the comment: code 7 needs a slot filled from the file)
    assert not re.search(r"^hipvoigtLBL!\(", j, re.M)                    # (no drop-in shape!: SpectralLines carries no shifts)


def test_python_refusals_before_device(cs, monkeypatch):
    """code 7 reads the slot's shifts: a table without a file is refused before any library call that would run a shape; the
    pressure_shift keyword on it is refused before any device call at all"""
    from clearsky_jl_amd import core
    assert core.needs_shifts(7) and core.needs_shifts(16) and not core.needs_shifts(6) and not core.needs_shifts(0)
    with pytest.raises(ValueError):
        core.shape_code("voigtLBL", True)
    with pytest.raises(ValueError):
        core.shape_code(7, True)
    assert core.shape_code("voigtLBL") == 7
    syn = cs.SpectralLines.synthetic(1, 20, 3, 0.0, 60.0)
    assert syn.source is None
    nu = np.linspace(1.0, 50.0, 11)

    def no_device(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(core, "default_context", no_device)
    monkeypatch.setattr(core, "lib", no_device)
    Om = cs.AtmosphericDomain((150.0, 350.0), 4, (10.0, 1e5), 4)
    for call in (lambda: cs.shape_batch(syn, "voigtLBL", nu, [296.0], [1e5], [40.0]),
                 lambda: cs.shape_points(syn, "voigtLBL", nu, [296.0], [1e5], [40.0]),
                 lambda: cs.voigtLBL(nu, syn, 296.0, 1e5, 40.0),
                 lambda: cs.voigtLBL(7.0, syn, 296.0, 1e5, 40.0),
                 lambda: cs.voigtLBL_(np.zeros_like(nu), nu, syn, 296.0, 1e5, 40.0),
                 lambda: cs.DirectGas(syn, 0.01, nu, shape="voigtLBL"),
                 lambda: cs.Gas(syn, 0.01, nu, Om, shape="voigtLBL")):
        with pytest.raises(ValueError, match="\\.par"):
            call()
    sl = cs.SpectralLines(os.path.join(HITRAN, "CO2.par"))
    g = cs.DirectGas(sl, 0.01, nu, shape="voigtLBL")   # a file-backed table is accepted, with the usual cut-off
    assert g.dnu_cut == 25.0 and cs.SHAPES[g.shape] == 7 and not g.pressure_shift
    with pytest.raises(ValueError):
        cs.voigtLBL(nu, sl, 296.0, 1e5, 40.0, pressure_shift=True)
    with pytest.raises(ValueError):
        cs.DirectGas(sl, 0.01, nu, shape="voigtLBL", pressure_shift=True)


def test_restatement_vs_40_digits(cs, O, case, capsys):
    """voigt_lbl_ref.expected on one-line slices against voigt_lbl_ref.sigma_line (40 digits): lines below and above the cut-off, every
    state of the device cases, points at the shifted centre, inside, at both direct edges and the mirror edge (exact there: dyadic) and
    beyond; both pre-filters.  Then the golden H2O file's own shifts at an arbitrary pressure."""
    T, P, Pp = V.states()
    worst = 0.0
    for cut in (1.0, 5.0, 25.0):
        for l in (0, 3, 40, 41, 150, len(case.nu) - 1):
            one = V.subset(case, np.arange(len(case.nu)) == l)
            one.delta_a = case.delta_a[l:l + 1]
            line = LP.line_of(one, 0)
            for k in range(len(T)):
                c = case.nu[l] + case.delta_a[l] * P[k] / KATM
                pts = np.unique(np.array([x for x in (c, c + 0.25, c - 0.5, c + cut, c - cut, cut - c, c + cut + 0.25, cut - c - 0.25,
                                                      cut - c + 0.25, 0.5, 64.5) if 0.0 < x]))
                for strict in (True, False):
                    val, scale = V.expected(cs, O, one, one.delta_a, pts, T[k], P[k], Pp[k], cut, strict)
                    for i, x in enumerate(pts):
                        e, sc = V.sigma_line(x, line, T[k], P[k], Pp[k], cut, ends=(pts[0], pts[-1]) if strict else None)
                        if sc == 0.0:
                            assert val[i] == 0.0 and scale[i] == 0.0, (cut, l, k, x)
                            continue
                        assert abs(scale[i] - sc) < 1e-12 * sc
                        worst = max(worst, abs(val[i] - e) / sc)
    h2o = cs.SpectralLines(os.path.join(HITRAN, "H2O.par"), numin=0.0, numax=150.0)
    wf = 0.0
    for l in (1, 5, 12, 30):
        one = V.subset(h2o, np.arange(len(h2o.nu)) == l)
        one.delta_a = h2o.delta_a[l:l + 1]
        line = LP.line_of(one, 0)
        Tq, Pq, Ppq = 251.3, 87654.3, 1234.5
        c = h2o.nu[l] + h2o.delta_a[l] * Pq / KATM
        pts = np.unique(np.array([x for x in (c + 0.013, c - 0.4, c + 24.9, 25.0 - c - 0.01, 0.37) if x > 0.0]))
        val, scale = V.expected(cs, O, one, one.delta_a, pts, Tq, Pq, Ppq, 25.0, False)
        for i, x in enumerate(pts):
            e, sc = V.sigma_line(x, line, Tq, Pq, Ppq, 25.0)
            if sc > 0.0:
                wf = max(wf, abs(val[i] - e) / sc)
    with capsys.disabled():
        print(f"\nvoigt_lbl_ref.expected against 40 digits: worst ratio {worst:.2e} (exact shifts), {wf:.2e} (the file's shifts)")
    assert worst < 1e-12 and wf < 1e-12, (worst, wf)


def test_sigma_isolated_code_7_is_sigma_line(cs, case):
    """lineparam_ref.sigma_isolated(7, ...), the reference of the per-line harnesses, equals voigt_lbl_ref.sigma_line as floats: at the
    shifted centre, inside, at both direct edges and the mirror edge, and beyond, every state of the device cases, and on the golden
    H2O file's shifts at an arbitrary pressure; its bound's centre term is there exactly where a term hangs on a shifted centre"""
    T, P, Pp = V.states()
    n = 0
    for cut in (1.0, 25.0):
        for l in (0, 3, 41, len(case.nu) - 1):
            line = LP.line_of(case, l)
            assert line["delta"] == case.delta_a[l]
            for k in range(len(T)):
                c = case.nu[l] + case.delta_a[l] * P[k] / KATM
                for x in (c, c + 0.25, c - 0.5, c + cut, c - cut, cut - c, c + cut + 0.25, cut - c - 0.25, cut - c + 0.25, 0.5, 64.5):
                    if x <= 0.0:
                        continue
                    a, sc = V.sigma_line(x, line, T[k], P[k], Pp[k], cut, C=0.37)
                    b, _, info = LP.sigma_isolated(7, x, line, T[k], P[k], Pp[k], cut, C=0.37)
                    assert a == b, (cut, l, k, x, a, b)
                    assert info["voigt"] and info["planck_T"] == 0.0 and (0.0 <= info["rel"] <= 1.0)
                    # dyadic: nothing but the centre's own rounding, and that only with a shift and a term in reach
                    # (at x = c the direct profile's slope is 0)
                    if not (sc > 0.0 and case.delta_a[l] * P[k] != 0.0):
                        assert info["centre"] == 0.0, (cut, l, k, x)
                    elif x != c:
                        assert info["centre"] > 0.0, (cut, l, k, x)
                    n += 1
    h2o = cs.SpectralLines(os.path.join(HITRAN, "H2O.par"), numin=0.0, numax=150.0)
    Tq, Pq, Ppq = 251.3, 87654.3, 1234.5
    for l in (1, 5, 12, 30):
        line = LP.line_of(h2o, l)
        c = h2o.nu[l] + h2o.delta_a[l] * Pq / KATM
        for x in (c + 0.013, c - 0.4, c + 24.9, 25.0 - c - 0.01, 0.37):
            if x > 0.0:
                a, sc = V.sigma_line(x, line, Tq, Pq, Ppq, 25.0)
                b, _, info = LP.sigma_isolated(7, x, line, Tq, Pq, Ppq, 25.0)
                assert a == b and (info["centre"] > 0.0) == (sc > 0.0), (l, x)
                n += 1
    assert n > 500


def test_premises_of_the_device_cases(cs, O, case):
    """Conditions the device cases rest on, on the reference alone"""
    nul, da, nu = case.nu, case.delta_a, V.GRID
    T, P, Pp = V.states()
    assert 280 <= len(nul) <= 420 and nul[0] > 0 and nul[-1] < 95.0
    assert set(np.unique(da)) <= set(V.DELTAS) and da.min() == -0.1875 and da.max() == 0.125
    assert np.any(np.sign(da[1:]) * np.sign(da[:-1]) < 0)
    assert len(P) == 9 and min(P) == 0.0 and max(P) == 2.0 * KATM and min(T) == 200.0 and max(T) == 320.0
    assert nu[0] < 1.0 and len(nu) == 257
    # a 25 cm^-1 window spans at least 3 blocks of 64 lines
    assert np.max(np.searchsorted(nul, nu + 25.0) - np.searchsorted(nul, nu - 25.0)) >= 3 * 64
    # dyadic exactness
    V.dyadic_premise(nul, nu, da, P)
    # membership by shifted centre against membership by table position
    count = dict(dir_in_lo=0, dir_in_hi=0, dir_out_lo=0, dir_out_hi=0, mir_in=0, mir_out=0)
    for cut in (1.0, 5.0, 25.0):
        for k in range(len(P)):
            d, m, d0, m0 = V.membership(nul, da, nu, P[k], cut)
            below = nul[None, :] < nu[:, None]
            count["dir_in_lo"] += int(np.sum(d & ~d0 & below)); count["dir_in_hi"] += int(np.sum(d & ~d0 & ~below))
            count["dir_out_lo"] += int(np.sum(~d & d0 & below)); count["dir_out_hi"] += int(np.sum(~d & d0 & ~below))
            count["mir_in"] += int(np.sum(m & ~m0)); count["mir_out"] += int(np.sum(~m & m0))
            if cut == 25.0 and k == 5:
                n25 = int(np.sum(d != d0) + np.sum(m != m0))
    assert all(v >= 1 for v in count.values()), count
    assert sum(count.values()) >= 20 and n25 >= 20, (count, n25)
    # cut = 0.25, below the largest shift (0.375): no table position is certainly inside, every candidate is fringe.  Pairs inside by
    # shifted centre but outside by table position, and the other way round, on both grids over the nine states (no mirror pair: both
    # grids start at or above 0.5)
    assert 0.25 < np.max(np.abs(da)) * max(P) / KATM
    for grid in (V.GRID, V.EDGE_GRID):
        V.dyadic_premise(nul, grid, da, P)
        n_in = n_out = 0
        for k in range(len(P)):
            d, m, d0, m0 = V.membership(nul, da, grid, P[k], 0.25)
            n_in += int(np.sum(d & ~d0)); n_out += int(np.sum(~d & d0))
            assert not m.any() and not m0.any()
        assert n_in > 0 and n_out > 0, (n_in, n_out)
    # an adjacent pair in shifted order reversed at the highest pressure, not at the lowest
    c_hi, c_lo = nul + da * max(P) / KATM, nul + da * min(P) / KATM
    assert np.any((np.diff(c_hi) < 0) & (np.diff(c_lo) > 0))
    # the strict pre-filter, the per-state one: some line is inside at some states only, at each grid end
    for lim in [V.EDGE_GRID[0] - D for D in (1.0, 5.0, 25.0)] + [nu[-1] + D for D in (1.0, 5.0, 25.0)]:
        side = np.array([[nul[j] + da[j] * p / KATM > lim for p in P] for j in range(len(nul))])
        assert np.any(side.any(axis=1) & ~side.all(axis=1)), lim
    # the shift matters: at P >= P0 / 4 the expected values differ from unshifted code 6 by more than 1e-6 at more than half the points
    for k in range(len(P)):
        if P[k] < 0.25 * KATM:
            continue
        a = V.expected(cs, O, case, da, nu, T[k], P[k], Pp[k], 25.0, True)[0]
        b = X.expected(cs, O, case, nu, T[k], P[k], Pp[k], 25.0, True)[0]
        assert np.mean(np.abs(a - b) > 1e-6 * np.abs(b)) > 0.5, k
    # P = 0: code 6, bit for bit on the reference
    a = V.expected(cs, O, case, da, nu, T[0], P[0], Pp[0], 25.0, True)
    b = X.expected(cs, O, case, nu, T[0], P[0], Pp[0], 25.0, True)
    assert np.array_equal(a[0], b[0])
