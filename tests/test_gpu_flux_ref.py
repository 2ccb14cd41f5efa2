"""Every flux kernel form against the 40-digit reference of tests/flux_ref.py, element by element: tau, M+ and M- each within
flux_ref.bounds(..., "device") at factor 1, exact zeros where the reference has exact zeros.  Nothing here compares the device with
itself or with the oracle, except the band-sum identity at the end (the run's own planes are its input; the sum is exact arithmetic).

Carrying sigma exactly.  The cross-section plane of flux_ref.case goes in as a function absorber (sigma_extra), looked up by node
pressure; there is no gray term.  The fused forms need a line gas: the CO2 fixture on a grid above its last line + 25 cm^-1 (asserted),
which contributes exact zeros.  Every run asserts that Column.sigma_nodes() is that plane bitwise, so the reference's input is exact
in every form and no form adds to the tau term of the bound.  Every run asserts the form it reports (info()["flux_form"]: 0 separate
kernels, 2 chunk, 3 scan; work()["dispatch"]["flags"]: RT_STREAMS, CHUNK4), as tests/test_gpu_flux_orders.py does.

  form                 how it is reached (cs_set_tuning)                NS       test
  k_rt<NS, true>       key 15 = 1, key 5 = 0                            1-16     stream_sweep, lobatto, boundaries, planck (key 5 = 0)
  k_rt_streams<NS>     key 15 = 1 (gray-only column: default keys)     2-8      stream_sweep, boundaries, planck
  k_flux_scan<NS, 5>   default keys                                     2-6      stream_sweep, boundaries, scan_chunks (per <= 5)
  k_flux_scan<NS, 0>   default keys NS 7, 8 or per = 6; key 15 | 2048   2-8      stream_sweep, boundaries, scan_chunks
  k_flux_chunk3<NS>    key 15 = 2, key 5 = 0                            1-16     stream_sweep, lobatto, boundaries
  k_flux_chunk<NS>     key 15 = 2 | 8, key 5 = 0                        1-16     stream_sweep, lobatto, boundaries
  k_rt<NS, false>      Column.run_batch, tiles x B >= 4096              1-16     batch (band fluxes of four members; B - 1: k_rt<NS, true>)
Every form is reached with the host-evaluated term.  What a run reports tells the forms apart, not the template instances of one
form: k_flux_scan<NS, 5> from <NS, 0> and k_rt<NS, true> from <NS, false> are inferred from the rules of flux_plan
(restated in flux_ref.scan_per and in test_batch) and from key 15 | 2048, as in tests/test_gpu_flux_orders.py.  Grid: 64 x 2 + 17 = 145 points (three tiles, a ragged last one), all compared.
One reference per (NS, nlobatto, np, inputs), shared by the forms (flux_ref.reference).  The scan form's bound carries the roundings of
forming A I + B per chunk (bounds(per=)); per comes from flux_ref.scan_per, the formula of flux_plan.

Band sum.  For every form that returns planes, on test_gpu_flux_orders' 2577-point grid with its CO2 lines (41 blocks, 3 groups of
CS_FLUX_GROUP): |F - fsum(w_j M_j)| <= (n + 2) u sum |w_j M_j| per level, with M the run's own planes and n the longest chain of
additions, read from the reduction code (cs_kernels.h):
  wave_sum                 rocprim warp_reduce over 64 lanes: 6
  block_partial_waves      the waves of a block, in order: up to 3 (four tiles per block)
  k_freduce                one partial per thread below 256 blocks (added to 0.0: exact), then a tree of 8 levels
  flux_last_block_reduce   the blocks of a group in order: 15; the groups in order, eight at a time: ngrp = 3 here, counted 8
  n:  k_rt 6 + 3 + 8 = 17;  k_rt_streams 6 + 8 = 14;  scan 6 + 15 + 8 = 29;  chunk forms 6 + 3 + 15 + 8 = 32   (all far below nnu = 2577)
The two roundings beside n are the product w_j M_j on either side.  The library's trapezoid weights are checked against exact rational
arithmetic on nu.  With the M+- check above, this replaces "1e-11 of max F+" by a per-level statement.

Worst error / bound per form over every case of this module, measured on an MI355X (the tests print them, pytest -s); no form came near the bound, and no kernel needed a change:
  form                                  tau     M+      M-      band sum (F+- against the exact sum of the run's planes)
  k_rt<NS, true>                        0.31    0.51    0.49    0.10
  k_rt_streams<NS>                      0.30    0.51    0.49    0.11
  k_flux_scan (default keys)            0.30    0.52    0.55    0.08
  k_flux_scan<NS, 0> (key 15 | 2048)    0.30    0.51    0.51    0.08
  k_flux_chunk3<NS>                     0.31    0.51    0.49    0.08
  k_flux_chunk<NS>                      0.31    0.51    0.49    0.08
  k_rt<NS, false> / <NS, true>, batch   band fluxes against the reference's: 0.08 (a sum of 145 worst-case element bounds)
(The oracle's own worst ratio against bounds("libm") is 0.48, tests/test_flux_ref.py: the device's exponential is charged three times
libm's, and lands where libm does.)
"""
import math
from fractions import Fraction

import numpy as np
import pytest
from mpmath import mp, mpf

import clearsky_jl_amd
import flux_ref as F
from clearsky_jl_amd import DISPATCH_FLAGS
from test_gpu_flux_orders import N_SHORT, _lines
from test_gpu_flux_orders import _run as _run_lines

pytestmark = pytest.mark.gpu

RT_STREAMS, CHUNK4 = DISPATCH_FLAGS["RT_STREAMS"], DISPATCH_FLAGS["CHUNK4"]
U = F.U

# name: (tuning keys, flux_form, RT_STREAMS, CHUNK4, scan)
FORMS = {
    "k_rt": (((15, 1), (5, 0)), 0, False, False, False),
    "k_rt_streams": (((15, 1),), 0, True, False, False),
    "scan": ((), 3, False, False, True),
    "scan0": (((15, 2048),), 3, False, False, True),
    "chunk3": (((15, 2), (5, 0)), 2, False, False, False),
    "chunk": (((15, 2 | 8), (5, 0)), 2, False, True, False),
}
N_CHAIN = {"k_rt": 17, "k_rt_streams": 14, "scan": 29, "scan0": 29, "chunk3": 32, "chunk": 32}


def _forms_for(ns):
    inr = 2 <= ns <= 8
    return [f for f in FORMS if inr or f not in ("k_rt_streams", "scan", "scan0")]


def _absorber(c):
    """the case's plane as a function absorber sigma(nu, T, P): row k for the node whose pressure is P"""
    row = {float(p): k for k, p in enumerate(c["Pk"])}
    assert len(row) == c["K"]
    return lambda v, T, P: c["sigma"][row[float(P)]]


def _run(c, tune=(), lines=True):
    """one column run of the case: outputs, the form it reports"""
    cs = clearsky_jl_amd
    nu = c["nu"]
    members = []
    if lines:
        g = cs.DirectGas(_lines("CO2"), 400e-6, nu)
        assert g.sl.nu.max() + 25.0 < nu[0]
        members.append(g)
    else:
        members.append(cs.GrayGas(0.0, nu))           # (carries the grid; no gray term)
    members.append(_absorber(c))
    ctx = cs.Context(0)
    try:
        for k, v in tune:
            ctx.set_tuning(k, v)
        col = cs.Column(c["P"], c["g"], c["T"], F.fmu, c["fS"], c["fa"], *members, core=cs.Discretized(c["ns"], c["nlob"]),
                        theta_s=c["theta_s"], ctx=ctx, _warn=False)
        for a, b in ((col.Tlev, c["Tlev"]), (col.muk, c["muk"]), (col.wts, cs.trapz_weights(nu))):
            assert np.array_equal(a, b)
        for a, b in ((col.S_toa, c["S_toa"]), (col.albedo, c["albedo"])):
            assert (a is None and b is None) or np.array_equal(a, b)
        assert col.sigma_gray == 0.0
        col.run()
        tau = np.zeros((col.nl, col.nnu), order="F")
        Mu = np.zeros((col.np, col.nnu), order="F")
        Md = np.zeros((col.np, col.nnu), order="F")
        Fup, Fdn = col.fetch(tau, Mu, Md)
        r = dict(tau=tau, Mup=Mu, Mdn=Md, Fup=Fup, Fdn=Fdn, form=col.info()["flux_form"], flags=col.work()["dispatch"]["flags"],
                 sigma=col.sigma_nodes())
    finally:
        ctx.close()
    return r


def _check(c, ref, form, label, lines=True, tune=None):
    """run the case in `form`, assert the form and the bitwise plane, hold tau, M+, M- to the bound"""
    keys, ff, streams, chunk4, scan = FORMS[form]
    r = _run(c, keys if tune is None else tune, lines)
    assert r["form"] == ff, (form, r["form"])
    assert bool(r["flags"] & RT_STREAMS) == streams and bool(r["flags"] & CHUNK4) == chunk4, (form, r["flags"])
    assert np.array_equal(r["sigma"], c["sigma"]), form
    nl = len(c["P"]) - 1
    b = F.bounds(ref, "device", per=F.scan_per(nl) if scan else None)
    rr = F.ratios(r, ref, b)
    print("\n  %s %s: worst error / bound  tau %.3f  M+ %.3f  M- %.3f" % (label, form, rr["tau"], rr["Mup"], rr["Mdn"]))
    if not F.within(rr):
        _FAILED.append((label, form, rr))              # (asserted when the test ends: every form of the case is run and printed first)
    return r


_FAILED = []


@pytest.fixture(autouse=True)
def _within_bound():
    """every form a test ran lay within the bound"""
    del _FAILED[:]
    yield
    assert not _FAILED, _FAILED


def _case(**kw):
    c = F.case(clearsky_jl_amd, **kw)
    assert F.planck_clear_of_overflow(c)
    return c


@pytest.mark.parametrize("ns", range(1, 17))
def test_stream_sweep(ns):
    """every NS in every form: profile (a), a beam of the order of the thermal emission, the albedo function; nlobatto 3, np 9 (K = 17)"""
    c = _case(prof="a", ns=ns, nlob=3, np_=9, fS="thermal", fa="fun", theta=0.6)
    ref = F.reference(("sweep", ns), c)
    for form in _forms_for(ns):
        if form == "scan0" and ns >= 7:
            continue                                    # (default keys already run <NS, 0>)
        _check(c, ref, form, "NS %d" % ns)


@pytest.mark.parametrize("nl", [20, 21, 40, 41, 60, 61])
def test_scan_chunks(nl):
    """the scan form at NS = 4 with 4, 8 and 12 waves, up to 5 layers per wave (<4, 5>; key 15 | 2048: <4, 0>) and 6 (<4, 0>)"""
    assert (F.scan_waves(nl), F.scan_per(nl)) == {20: (4, 5), 21: (8, 3), 40: (8, 5), 41: (12, 4), 60: (12, 5), 61: (12, 6)}[nl]
    c = _case(prof="a", ns=4, nlob=2, np_=nl + 1, fS="thermal", fa="fun", theta=0.6)
    ref = F.reference(("scan", nl), c)
    _check(c, ref, "scan", "nl %d" % nl)
    if F.scan_per(nl) <= 5:
        _check(c, ref, "scan0", "nl %d" % nl)


@pytest.mark.parametrize("nlob", [2, 5, 16])
def test_lobatto(nlob):
    """the chunk forms and k_rt at NS = 4: nlobatto 2, 5 (nlob - 1 does not divide the 16-state loads), 16"""
    c = _case(prof="c", ns=4, nlob=nlob, np_=9, fS="thermal", fa="fun", theta=0.6)
    ref = F.reference(("lob", nlob), c)
    for form in ("k_rt", "chunk3", "chunk"):
        _check(c, ref, form, "nlob %d" % nlob)


@pytest.mark.parametrize("n", range(len(F.BOUNDARIES)))
def test_profiles_and_boundaries(n):
    """every boundary setting (beam none / zeros / positive / faint, albedo none / 0 / function / 1 / faint, theta_s 0 / 0.6 / 1.5) and
    every profile, in every form, NS = 4"""
    fS, fa, th = F.BOUNDARIES[n]
    prof = "abc"[n % 3]
    c = _case(prof=prof, ns=4, nlob=3, np_=9, fS=fS, fa=fa, theta=th)
    ref = F.reference(("bnd", n), c)
    for form in FORMS:
        _check(c, ref, form, "%s %s %s %.1f" % (prof, fS, fa, th))


def test_profile_coverage():
    assert {"abc"[n % 3] for n in range(len(F.BOUNDARIES))} == {"a", "b", "c"}


@pytest.mark.parametrize("fS,fa", [("pos", "fun"), ("none", "none")])
def test_planck_regimes(fS, fa):
    """columns without a line gas (form 0: k_rt_streams by default, k_rt with key 5 = 0) on a log grid from 1e-3 cm^-1 (Rayleigh-Jeans:
    exp(x) - 1 at x = 5e-6) through 1e5 to 4e5 cm^-1, where exp overflows at every level: B = 0 there, and M+- are exactly the stellar
    and reflected terms (exact zeros without them)"""
    nu = np.concatenate([np.logspace(-3.0, 5.0, F.NNU_GPU - 5), [1.1e5, 1.3e5, 2e5, 3e5, 4e5]])
    c = _case(prof="a", ns=4, nlob=3, np_=9, fS=fS, fa=fa, theta=0.6, nu=nu)
    x = F.planck_x_double(nu[None, :], c["Tlev"][:, None])
    dark = np.all(x > F.LN_DBL_MAX, axis=0)
    assert dark.sum() >= 3 and np.any((x > F.LN_DBL_MAX).any(axis=0) & ~dark) and x.min() < 1e-5
    ref = F.reference(("planck", fS), c)
    for form, tune in (("k_rt_streams", ()), ("k_rt", ((5, 0),))):
        r = _check(c, ref, form, "planck " + fS, lines=False, tune=tune)
        if fS == "none":
            assert np.all(r["Mup"][:, dark] == 0.0) and np.all(r["Mdn"][:, dark] == 0.0)


# ---- batch: k_rt<NS, false> ------------------------------------------------------------------------------------------------------

def _member(b, B):
    """temperature (levels) and molar mass of batch member b: both differ from member to member"""
    f = b / B
    return (lambda p: 200.0 + (85.0 + 10.0 * f) * (p / 1e5) ** (0.19 + 0.05 * f)), (lambda T, P: 0.029 - (0.001 + 0.002 * f) * (P / 1e5))


@pytest.mark.parametrize("ns", range(1, 17))
def test_batch(ns):
    """Column.run_batch on a gray column, tiles x B at the 4096 rule (k_rt<NS, false>) and one below it (k_rt<NS, true>): the band
    fluxes of members 0, 1, the middle one and B - 1 against sum_j w_j M_j of the reference over all 145 points, within
    sum_j w_j bound_j + (n + 2) u sum_j |w_j M_j|, n = 17 (k_rt).  Which of the two instances runs is inferred from the rule of
    flux_plan (restated here: fewer than 4096 (tile, column) waves -> two waves per tile), not reported by the library; the run only
    reports that k_rt_streams did not take it.  The column's own run hands back the gray plane bitwise"""
    cs = clearsky_jl_amd
    nlob, np_, sig = 2, 7, 3e-27
    nu = np.linspace(600.0, 760.0, F.NNU_GPU)
    tiles = -(-len(nu) // 64)
    B = -(-4096 // tiles)
    assert tiles * B >= 4096 > tiles * (B - 1)
    P = cs.pressuregrid(5.0, 1e5, np_)
    ctx = cs.Context(0)
    try:
        col = cs.Column(P, F.G, _member(0, B)[0], _member(0, B)[1], lambda v: 0.1 + 0.05 * math.sin(v / 37.0), F.albedo_of("fun"),
                        cs.GrayGas(sig, nu), core=cs.Discretized(ns, nlob), theta_s=0.6, ctx=ctx, _warn=False)
        col.run()
        assert np.array_equal(col.sigma_nodes(), np.full((col.K, len(nu)), sig))
        Ts, mus = [_member(b, B)[0] for b in range(B)], [_member(b, B)[1] for b in range(B)]
        out = {}
        for nb in (B, B - 1):
            out[nb] = col.run_batch(Ts[:nb], mus[:nb])
            assert not col.work()["dispatch"]["flags"] & RT_STREAMS
        S_toa, albedo, wts = col.S_toa, col.albedo, col.wts
    finally:
        ctx.close()
    m, W = cs.streamnodes(ns)
    ws = cs.lobattonodes(nlob)[1]
    K = (np_ - 1) * (nlob - 1) + 1
    worst = 0.0
    for b in (0, 1, B // 2, B - 1):
        fT, fm = _member(b, B)
        Tn, mun = cs.core.lobattoevaluations(P, fT, fm, nlob)
        Tlev = np.array([fT(p) for p in P])
        ref = F.mp_fluxes(nu, P, F.G, cs.core.nodevalues(mun, nlob), Tlev, np.full((K, len(nu)), sig), S_toa, albedo, 0.6, ws, m, W,
                          detail=True)
        bnd = F.bounds(ref, "device")
        with mp.workdps(40):
            for key, plane in (("Fup", "Mup"), ("Fdn", "Mdn")):
                Fref = [mp.fsum(mpf(float(w)) * x for w, x in zip(wts, ref[plane][i])) for i in range(np_)]
                eF = (wts[None, :] * bnd[plane]).sum(axis=1) + (17 + 2) * U * (wts[None, :] * np.abs(ref["detail"][plane])).sum(axis=1)
                for nb in (B, B - 1):
                    if b >= nb:
                        continue
                    got = out[nb][0 if key == "Fup" else 1][b]
                    assert np.all(np.isfinite(got)), (ns, b, nb, key)
                    err = np.array([float(abs(mpf(float(got[i])) - Fref[i])) for i in range(np_)])
                    worst = max(worst, float(np.max(err / eF)))
                    assert np.all(err <= eF), (ns, b, nb, key, err / eF)
    print("\n  batch NS %d: worst error / bound of the band fluxes %.3f" % (ns, worst))


# ---- the band sum ----------------------------------------------------------------------------------------------------------------

def test_trapezoid_weights_exact():
    """the weights the column hands to the device against exact rational arithmetic on nu: two differences, one sum -- 2 u"""
    cs = clearsky_jl_amd
    for nu in (np.linspace(600.0, 760.0, N_SHORT), np.linspace(F.NU_LO, F.NU_HI, F.NNU_GPU), np.logspace(-3.0, 5.0, 140)):
        w = cs.trapz_weights(nu)
        q = [Fraction(float(v)) for v in nu]
        for j in range(len(nu)):
            ex = ((q[j] - q[j - 1] if j else 0) + (q[j + 1] - q[j] if j + 1 < len(nu) else 0)) / 2
            assert abs(Fraction(float(w[j])) - ex) <= Fraction(2 * U) * ex, j


@pytest.mark.parametrize("ns", range(1, 17))
def test_band_sum(ns):
    """the stream-sweep cases of test_gpu_flux_orders (2577 points, real CO2 lines, 41 blocks): F+- against the exact sum of the
    run's own planes, (n + 2) u sum |w_j M_j| per level"""
    cs = clearsky_jl_amd
    w = cs.trapz_weights(np.linspace(600.0, 760.0, N_SHORT))
    for form in _forms_for(ns):
        keys, ff, streams, chunk4, _ = FORMS[form]
        r = _run_lines(ns, 3, N_SHORT, 9, keys)
        assert r["form"] == ff and bool(r["flags"] & RT_STREAMS) == streams and bool(r["flags"] & CHUNK4) == chunk4, (form, r["form"])
        assert np.array_equal(r["col"].wts, w)
        worst = 0.0
        for key, plane in (("Fup", "Mup"), ("Fdn", "Mdn")):
            for i in range(9):
                prod = w * r[plane][i]
                exact = math.fsum(prod)
                lim = (N_CHAIN[form] + 2) * U * math.fsum(np.abs(prod))
                err = abs(r[key][i] - exact)
                assert math.isfinite(r[key][i]) and math.isfinite(exact), (form, key, i)
                worst = max(worst, err / lim if lim else (0.0 if err == 0 else math.inf))
                assert err <= lim, (form, key, i, err, lim)
        print("\n  band sum NS %d %s: worst error / bound %.3f" % (ns, form, worst))
