"""CPU tests of tests/depth_ref.py -- the per-element bound of the column depth and of the tile transmittances is neither too tight
nor idle -- and of the host side of the two modes: the header's names, tau_mode, band_transmittance, the Julia binding.  No GPU.

  * the plain-double numpy restatement lies within the bound at factor 1 on flux_ref's planes: S_FULL (column depths from 7e-8, every
    layer below dDepth!'s floor, to 9e3) and S_THICK, theta 0 and 0.6, nlobatto 2, 3 and 4, np 2 and 9 (24 cases of 145 points).
  * the bound rejects each planted fault.  Faults that cannot show in a case are not asked of it: the slant factor at theta = 0
    (m = 1), the unshared end node on one layer (np = 2: there is no second layer), the floor on S_THICK (no layer below it).  Every
    fault is rejected in at least the S_FULL, np = 9, theta = 0.6 cases of all three orders.
  * sharpness: the bound of D is below 1e-13 of the value in every element.  A tile sum's bound holds the exponential's conditioning,
    D rel_D per term, which alone passes 1e-13 where a tile's terms all have D > 40: the criterion is asked of the elements whose
    weighted mean depth sum(w e^-D D) / sum(w e^-D) is at most 30 -- every element of the S_FULL cases (each tile holds transparent
    points) and the upper levels of S_THICK -- and there it is below 1e-13 of the value.
"""
import math
import re

import numpy as np
import pytest

import depth_ref as DR
import flux_ref as F
import test_julia_binding as JB

SETS = {"full": F.S_FULL, "thick": F.S_THICK}
CASES = [(s, th, nlob, np_) for s in SETS for th in (0.0, 0.6) for nlob in (2, 3, 4) for np_ in (2, 9)]
_IDS = ["%s-th%.1f-lob%d-np%d" % c for c in CASES]
_DONE = {}


def _case(cs, c):
    if c not in _DONE:
        s, th, nlob, np_ = c
        k = DR.case(cs, nlob, np_, theta=th, sset=SETS[s])
        w = cs.trapz_weights(k["nu"])
        a = dict(P=k["P"], g=k["g"], muk=k["muk"], sigma=k["sigma"], theta_s=th, ws=k["ws"])
        ref = DR.mp_depth(wts=w, **a)
        _DONE[c] = (a, w, ref, DR.bounds(ref))
    return _DONE[c]


def test_planes_span_the_regimes(cs):
    a, w, ref, bnd = _case(cs, ("full", 0.0, 3, 9))
    D = F.to_float(ref["D"])
    assert D[-1].min() < 1e-7 and 5e3 < D[-1].max() < 2e4          # far below nl x 1e-6 = 8e-6: the floor would show
    assert np.all(np.diff(D, axis=0) > 0.0) and np.all(D[0] == 0.0)
    T = F.to_float(ref["T"])
    assert T.shape == (9, 3) and np.all(np.diff(T, axis=0) < 0.0)
    assert [float(x) for x in T[0]] == pytest.approx([math.fsum(w[j0:j1]) for j0, j1 in DR.tile_ranges(len(w))], rel=1e-15)


@pytest.mark.parametrize("c", CASES, ids=_IDS)
def test_restatement_within_the_bound(cs, c):
    a, w, ref, bnd = _case(cs, c)
    got = DR.np_depth(wts=w, **a)
    rr = DR.ratios(got, ref, bnd)
    print("  ", c, {k: "%.3f" % v for k, v in rr.items()})
    assert set(rr) == {"D", "T"} and all(v <= 1.0 for v in rr.values()), rr


def _shows(fault, c):
    s, th, nlob, np_ = c
    if fault == "m":
        return th != 0.0
    if fault == "end_node":
        return np_ > 2
    if fault == "floor":
        return s == "full"
    return True


@pytest.mark.parametrize("fault", DR.FAULTS)
def test_bound_rejects_the_planted_fault(cs, fault):
    seen = 0
    for c in CASES:
        if not _shows(fault, c):
            continue
        a, w, ref, bnd = _case(cs, c)
        rr = DR.ratios(DR.np_depth(wts=w, fault=fault, **a), ref, bnd)
        key = "T" if fault in ("weights", "tile_edge") else "D"
        assert rr[key] > 1.0, (fault, c, rr)
        if fault not in ("weights", "tile_edge"):
            assert c[0] != "full" or rr["T"] > 1.0, (fault, c, rr)   # a wrong depth is a wrong transmittance (S_THICK: where any is left)
        else:
            assert rr["D"] <= 1.0, (fault, c, rr)
        seen += 1
    assert seen >= 6, fault


@pytest.mark.parametrize("c", CASES, ids=_IDS)
def test_bound_is_sharp(cs, c):
    a, w, ref, bnd = _case(cs, c)
    D, T, DT = F.to_float(ref["D"]), F.to_float(ref["T"]), F.to_float(ref["DT"])
    assert np.all(bnd["D"][1:] <= 1e-13 * D[1:]) and np.all(bnd["D"][0] == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ask = (T > 0.0) & (DT <= 30.0 * T)
    assert np.all(bnd["T"][ask] <= 1e-13 * T[ask])
    assert np.all(ask[0]) and (c[0] != "full" or np.all(ask)), c


def test_ratio_fails_on_a_nan(cs):
    a, w, ref, bnd = _case(cs, ("full", 0.6, 2, 9))
    got = DR.np_depth(wts=w, **a)
    got["D"][3, 5] = np.nan
    assert DR.ratios(got, ref, bnd)["D"] == math.inf


def test_host_formula_is_the_last_row(cs):
    a, w, ref, bnd = _case(cs, ("full", 0.6, 4, 9))
    h = DR.host_formula(a["P"], a["g"], a["muk"], a["sigma"], 0.6, a["ws"])
    assert np.array_equal(h, DR.np_depth(wts=w, **a)["D"][-1])


# ---- the host side of the two modes ------------------------------------------------------------------------------------------------

def test_header_names_the_values_of_want_tau():
    src = open(JB.HEADER).read()
    vals = dict(re.findall(r"^#define (CS_TAU_\w+)\s+(\d+)\b", src, flags=re.M))
    assert vals == {"CS_TAU_NONE": "0", "CS_TAU_LAYERS": "1", "CS_TAU_TOTAL": "2", "CS_TAU_TILES": "3"}
    assert len(JB.header_prototypes()) == 48          # macros only: the ABI gained no prototype
    flat = " ".join(src.split())
    for needle in ("CS_TAU_TOTAL [nnu]", "CS_TAU_TILES [np, ntile]", "there is no floor here", "k_depth"):
        assert needle in flat, needle


def test_python_modes_follow_the_header(cs):
    from clearsky_jl_amd import core
    assert (core.TAU_NONE, core.TAU_LAYERS, core.TAU_TOTAL, core.TAU_TILES) == (0, 1, 2, 3)
    assert [cs.tau_mode(x) for x in (False, None, 0, True, 1, "total", "tiles")] == [0, 0, 0, 1, 1, 2, 3]
    for bad in ("layers", "edges", ""):
        with pytest.raises(ValueError):
            cs.tau_mode(bad)


def test_band_transmittance(cs):
    rng = np.random.default_rng(11)
    npl, ntile = 5, 41
    Tt = np.sort(rng.random((npl, ntile)), axis=0)[::-1].copy()
    edges = [0, 3, 4, 40, ntile]
    B = cs.band_transmittance(Tt, edges)
    assert B.shape == (npl, 4) and np.all(B[0] == 1.0)
    for q, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        for i in range(npl):
            assert B[i, q] == math.fsum(Tt[i, a:b]) / math.fsum(Tt[0, a:b])
    assert np.all(np.diff(B, axis=0) <= 0.0)


@pytest.mark.parametrize("edges", [[0, 2.5, 41], [0, 42], [-1, 3], [0, 5, 5, 41], [0, 7, 3], [4], [[0, 1], [2, 3]]])
def test_band_transmittance_refuses_what_band_fluxes_refuses(cs, edges):
    with pytest.raises(ValueError):
        cs.band_transmittance(np.ones((3, 41)), edges)


def test_band_transmittance_refuses_other_shapes(cs):
    with pytest.raises(ValueError):
        cs.band_transmittance(np.ones(41), [0, 1])


def test_multicontext_and_accessors_refuse(cs):
    mc = object.__new__(cs.MultiContext)              # (no device behind it: the refusal must come first)
    mc.ctxs = []
    nu = np.linspace(600.0, 700.0, 130)
    P = cs.pressuregrid(10.0, 1e5, 4)
    gas = cs.GrayGas(1e-27, nu)
    for mode in ("total", "tiles"):
        with pytest.raises(TypeError, match="cs_fluxes_discretized_multi"):
            cs.Column(P, 9.8, np.full(4, 250.0), 0.029, None, None, gas, want_tau=mode, ctx=mc)
    with pytest.raises(ValueError):
        cs.Column(P, 9.8, np.full(4, 250.0), 0.029, None, None, gas, want_tau="layers", ctx=mc)
    # the accessors look at the column's mode before anything else (no device behind these columns either)
    for want, fn in ((True, "column_depth"), ("tiles", "column_depth"), (False, "tile_transmittance"), ("total", "tile_transmittance")):
        col = object.__new__(cs.Column)
        col.want_tau, col.tau_mode = want, cs.tau_mode(want)
        with pytest.raises(TypeError, match="want_tau="):
            getattr(col, fn)()


def test_julia_binds_the_depth_mode():
    src = open(JB.JL).read()
    for name in ("hipopticaldepth", "hiptransmittance"):
        assert f"function {name}(" in src and re.search(r"^export .*(\n.*)*" + name, src, flags=re.M), name
    start = src.index("function hipopticaldepth(")
    body = src[start:src.index("\nend", src.index("function hiptransmittance(", start))]
    calls = JB.julia_ccalls(body)
    JB._check_calls(calls, JB.header_prototypes(), "julia/ClearSkyHIP.jl: hipopticaldepth")
    used = [c[0] for c in calls]
    for sym in ("cs_column_setup", "cs_column_sigma_run", "cs_column_fetch"):
        assert sym in used, sym
    assert used.index("cs_column_setup") < used.index("cs_column_sigma_run") < used.index("cs_column_fetch")
    assert "cs_column_run" not in used                               # no sweep
    # every ccall of the file names a declared symbol
    protos = JB.header_prototypes()
    assert {c[0] for c in JB.julia_ccalls(src)} <= set(protos)
