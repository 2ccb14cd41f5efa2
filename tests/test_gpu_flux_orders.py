"""Every form of the flux stage at every stream count (1..16) and Lobatto order (2..16) the C ABI accepts, against the oracle and against
a second form on the same grid.

The flux kernels are templated on the stream count; from NS = 9 the compiler lays k_rt out differently (93 -> 146 VGPRs) and
k_flux_chunk3 spills, so the instances are not copies of the tested ones.  Every case asserts the form the library reports
(Column.info()["flux_form"]: 0 separate kernels, 2 chunk, 3 scan; Column.work()["dispatch"]["flags"]: RT_STREAMS = 4, CHUNK4 = 32),
compares with the oracle at the suite's tolerances (sigma and tau 1e-11 relative, M+- 1e-11 of their maximum plus
conftest.source_rounding_bound, F+- 1e-11 of max F+; columns with a CIA pair 1e-10, as test_gpu_flux_fused) and with a second form:
bitwise where an existing test documents identical results, else test_gpu_merge._close(..., 5e-13, 1e-12).  Forms are forced only by the
existing cs_set_tuning keys (5, 15 and its bits 2, 8, 2048).  Grid-size rules are taken from their formulas in cs_api.hip (flux_plan),
so a moved threshold fails here instead of leaving a form unrun.

Inputs: HITRAN CO2 fixture line by line, a gray term, a stellar beam (theta_s = 0.6), an albedo function; a CIA pair (CO2-CO2) in part
of the cases; 2577-point grids (41 tiles, a last tile of 17 points) unless a rule needs another.

  form                          how it is reached                                   NS       test
  k_rt<NS, true>                key 15 = 1, key 5 = 0 (short grid: < 4096 waves)    1-16     test_stream_sweep
                                default keys, NS outside 2-8                        1, 9-16  test_stream_sweep (bitwise the above)
  k_rt_streams<NS>              key 15 = 1 (<= 400 tiles); gray-only column         2-8      test_stream_sweep
                                (NS 1, 9-16: flag clear, k_rt<NS, true> runs)
  k_rt<NS, false>               Column.run_batch, tiles x B >= 4096 (B one below:   1-16     test_stream_sweep_batch
                                k_rt<NS, true>)
  k_flux_scan<NS, 5>            default keys, nl <= 60 (per <= 5)                   2-6      test_stream_sweep, test_scan_per_rule
  k_flux_scan<NS, 0>            default keys NS 7-8; nl = 61 (per = 6);             2-8      test_stream_sweep, test_scan_per_rule
                                key 15 | 2048 (bitwise <NS, 5>)
  k_flux_chunk3<NS>             key 15 = 2, key 5 = 0                               1-16     test_stream_sweep
  k_flux_chunk<NS>              key 15 = 2 | 8, key 5 = 0                           1-16     test_stream_sweep

  (Key 15 = 2 alone keeps the scan form wherever k_rt_streams could run -- flux_plan takes the setup-time k_rt_streams choice as reason enough for the scan -- so on
  these short grids key 5 = 0 goes with it.)

  nlobatto 2..16, NS = 4: the scan form, k_flux_chunk3, k_rt<4, true> and the batch k_rt<4, false> (test_lobatto_sweep); K mod 16 takes
  many values; the orders whose nlob - 1 does not divide 16 put layers across two of the chunk form's 16-state loads; the near-line plane
  (key 7 = 2) and a CIA pair in part of them.
  LDS limits, both sides: the scan form (test_scan_lds_limit), k_rt_streams at NS = 8 (test_rt_streams_lds_limit), the chunk form with
  R = 16 + nlob - 1 rows (test_chunk_lds_limit); past each, form 0 and oracle parity.
  Entry points: cs_fluxes_discretized at Discretized(16, 16) (test_fluxes_discretized_16_16); nstream 0 / 17 and nlobatto 1 / 17 refused
  with CS_EINVAL by cs_column_setup, cs_fluxes_discretized and cs_fluxes_discretized_members (test_orders_outside_the_abi_refused).

Instances that no input reaches: k_flux_scan<NS, 5> for NS 7, 8 and k_flux_scan / k_rt_streams for NS 1, 9..16 are not instantiated
(`if constexpr` in launch_flux); flux_plan names form 3 and k_rt_streams only for 2 <= NS <= 8, which
test_stream_sweep asserts for every NS outside that range (launch_flux would refuse such a plan with CS_EINVAL).
"""
import functools
import os

import numpy as np
import pytest

import clearsky_jl_amd
import workloads as W
from clearsky_jl_amd import DISPATCH_FLAGS
from conftest import HITRAN, relerr, source_rounding_bound
from test_gpu_boundary import _julia_call
from test_gpu_dispatch import _first_n
from test_gpu_merge import _close

pytestmark = pytest.mark.gpu

RT_STREAMS, CHUNK4 = DISPATCH_FLAGS["RT_STREAMS"], DISPATCH_FLAGS["CHUNK4"]   # Column.work()["dispatch"]["flags"]
LIM = 160 * 1024 - 4096                          # LDS the flux forms may take (flux_plan)
N_SHORT = 64 * 40 + 17                           # 41 tiles, ragged last tile
THETA_S, FS, GRAY = 0.6, 0.4, 5e-27
CS_EINVAL = -1


def FA(v):
    return 0.05 + 0.3 * np.sin(v / 40.0) ** 2


def _fun(v, T_, P_):                            # (gray-only column: a function absorber so that the spectrum is not flat)
    return 2e-27 * (P_ / 1e5) * (np.asarray(v) / 700.0) ** 4


def _nu(n):
    return np.linspace(600.0, 760.0, n)


def _tiles(n):
    return -(-n // 64)


def _K(np_, nlob):
    return (np_ - 1) * (nlob - 1) + 1


# the grid-size rules, copied from cs_api.hip
def _ud(n, B=1):                                 # flux_plan: two waves per tile below 4096 (tile, column) waves
    return _tiles(n) * B < 4096


def _streams_sh(np_, ns):                        # flux_plan: k_rt_streams' LDS
    return ((2 * np_ - 1) * 64 + 4 * ns * 64 + 2 * np_ + 64) * 8


def _rt_streams(n, np_, ns, key5=1):
    return bool(key5) and _ud(n) and _tiles(n) <= 400 and 2 <= ns <= 8 and _streams_sh(np_, ns) <= LIM


def _scan_nw(nl):                                # flux_plan: waves of the scan form
    return min(12, max(4, 4 * ((nl + 19) // 20)))


def _scan_sh(np_, nlob, ns):
    return (_K(np_, nlob) * 64 + (2 * np_ - 1) * 64 + 2 * (ns + 1) * 64 + 2 * np_) * 8


def _scan_per(np_):                              # flux_plan: layers per wave
    nl = np_ - 1
    return -(-nl // _scan_nw(nl))


def _chunk_sh(np_, nlob):                        # flux_plan: the chunk form, four waves, R = 16 + nlob - 1 ring rows each
    return (2 * np_ * 4 + 4 * (16 + nlob - 1) * 64) * 8


@functools.lru_cache(maxsize=None)
def _lines(name):
    return clearsky_jl_amd.SpectralLines(os.path.join(HITRAN, name + ".par"))


@functools.lru_cache(maxsize=None)
def _cia_data():
    return clearsky_jl_amd.readcia(W.fixture("CO2-CO2_2018.cia"))


def _members(nu, cia=False, gray_only=False, cut=25.0):
    cs = clearsky_jl_amd
    m = []
    if not gray_only:
        m.append(cs.DirectGas(_lines("CO2"), 0.9 if cia else 400e-6, nu, dnu_cut=cut))
    if cia:
        m.append(cs.CIATables(W.fixture("CO2-CO2_2018.cia")))
    m.append(cs.GrayGas(GRAY, nu))
    if gray_only:
        m.append(_fun)
    return m


def _column(ns, nlob, n, np_, ctx, cia=False, gray_only=False, cut=25.0, **kw):
    cs = clearsky_jl_amd
    nu = _nu(n)
    P = cs.pressuregrid(5.0, 1e5, np_)
    return cs.Column(P, 9.8, W.earth_temperature(P), 0.029, FS, FA, *_members(nu, cia, gray_only, cut), core=cs.Discretized(ns, nlob),
                     theta_s=THETA_S, ctx=ctx, _warn=False, **kw)


@functools.lru_cache(maxsize=12)
def _run(ns, nlob, n, np_, tune=(), cia=False, gray_only=False, cut=25.0):
    """one column run with the given cs_set_tuning keys: every output, the form it reports, the column (for the oracle)"""
    cs = clearsky_jl_amd
    ctx = cs.Context(0)
    try:
        for k, v in tune:
            ctx.set_tuning(k, v)
        col = _column(ns, nlob, n, np_, ctx, cia, gray_only, cut)
        col.run()
        tau = np.zeros((col.nl, col.nnu), order="F")
        Mu = np.zeros((col.np, col.nnu), order="F")
        Md = np.zeros((col.np, col.nnu), order="F")
        Fup, Fdn = col.fetch(tau, Mu, Md)
        r = dict(sigma=col.sigma_nodes(), tau=tau, Mup=Mu, Mdn=Md, Fup=Fup, Fdn=Fdn, nu=col.nu, Tlev=col.Tlev, col=col,
                 form=col.info()["flux_form"], flags=col.work()["dispatch"]["flags"], streams=col.work()["dispatch"]["streams"], cia=cia)
    finally:
        ctx.close()
    return r


def _oracle(O, col, want_sigma=True):
    extra = col.sigma_extra.copy() if col.sigma_extra is not None else None
    if col.U.cia:
        extra = np.zeros((col.K, col.nnu)) if extra is None else extra
        for k in range(col.K):
            extra[k] += O.cia_sigma(_cia_data(), col.nu, col.Tk[k], col.Pk[k], col.cia_P1[0, k], col.cia_P2[0, k])
    return O.fluxes_discretized(col.nu, col.P, col.g, col.core.nlobatto, col.Tn, col.mun, col.Tlev, [g.sl for g in col.gases],
                                ["voigt"] * len(col.gases), list(col.cuts), col.conc, sigma_gray=col.sigma_gray, sigma_extra=extra,
                                S_toa=col.S_toa, albedo=col.albedo, theta_s=col.theta_s, nstream=col.core.nstream, want_sigma=want_sigma)


_REF = {}


def _ref(O, r, key):
    """the oracle of a run's column, kept for the other forms on the same grid (the oracle does not depend on the tuning keys)"""
    if key not in _REF:
        if len(_REF) > 4:
            _REF.clear()
        _REF[key] = _oracle(O, r["col"])
    return _REF[key]


def _vs_oracle(r, ref):
    cs = clearsky_jl_amd
    tol = 1e-10 if r["cia"] else 1e-11
    assert relerr(r["sigma"], ref["sigma"], floor=1e-300) < tol
    assert relerr(r["tau"], ref["tau"]) < tol
    sm = max(ref["Mup"].max(), ref["Mdn"].max())
    amp = source_rounding_bound(cs, r["nu"], r["Tlev"], ref["tau"])
    for k in ("Mup", "Mdn"):
        assert np.max(np.abs(r[k] - ref[k])) < tol * sm + amp, k
    fm = ref["Fup"].max()
    for k in ("Fup", "Fdn"):
        assert np.max(np.abs(r[k] - ref[k])) < tol * fm, k


def _same(a, b, bitwise):
    """bitwise: per-wavenumber outputs identical, band fluxes to the order in which block partials are added (1e-14), node
    cross-sections (evaluated again into HBM after a fused run) to 5e-13; else test_gpu_merge._close at 5e-13 / 1e-12 (a CIA pair:
    1e-12, the order of its bilinear interpolation, test_gpu_flux_fused)"""
    if not bitwise:
        tol = 1e-12 if a["cia"] else 5e-13
        _close(a, b, tol, 1e-12)
        return
    for k in ("tau", "Mup", "Mdn"):
        assert np.array_equal(a[k], b[k]), k
    fm = np.max(b["Fup"])
    for k in ("Fup", "Fdn"):
        assert np.max(np.abs(a[k] - b[k])) <= 1e-14 * fm, k
    assert relerr(a["sigma"], b["sigma"], floor=1e-300) < 5e-13


def _is(r, form, streams=False, chunk4=False):
    assert r["form"] == form, (r["form"], form)
    assert bool(r["flags"] & RT_STREAMS) == streams, r["flags"]
    assert bool(r["flags"] & CHUNK4) == chunk4, r["flags"]


# ---- a. every stream count in every form ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", range(1, 17))
def test_stream_sweep(O, ns):
    """k_rt<NS, true>, k_rt_streams<NS>, the default form (scan for 2..8, k_rt<NS, true> outside), k_flux_chunk3<NS>, k_flux_chunk<NS>
    on one grid (nlobatto 3, 8 layers: K = 17, one state past a 16-state load), then a gray-only column (flux_form 0: no gas) with and
    without k_rt_streams"""
    n, nlob, np_ = N_SHORT, 3, 9
    inr = 2 <= ns <= 8
    assert _ud(n) and _tiles(n) <= 400 and _scan_sh(np_, nlob, ns) <= LIM and _chunk_sh(np_, nlob) <= LIM
    assert _rt_streams(n, np_, ns) == inr
    A = _run(ns, nlob, n, np_, ((15, 1), (5, 0)))
    _is(A, 0)
    ref = _ref(O, A, ("sweep", ns))
    _vs_oracle(A, ref)
    B = _run(ns, nlob, n, np_, ((15, 1),))
    _is(B, 0, streams=inr)
    _vs_oracle(B, ref)
    _same(B, A, bitwise=not inr)                 # (outside 2..8 the same kernel runs)
    C = _run(ns, nlob, n, np_)
    _is(C, 3 if inr else 0, streams=False)       # (the scan form takes k_rt_streams' grids; outside 2..8 neither may run)
    if inr:
        assert _scan_per(np_) <= 5               # k_flux_scan<NS, 5> for NS <= 6, <NS, 0> for 7 and 8
    _vs_oracle(C, ref)
    _same(C, A, bitwise=not inr)
    D = _run(ns, nlob, n, np_, ((15, 2), (5, 0)))
    _is(D, 2)
    _vs_oracle(D, ref)
    _same(D, A, bitwise=True)                    # (chunk form = separate kernels: test_chunk_form_bitwise_vs_separate_kernels)
    E = _run(ns, nlob, n, np_, ((15, 2 | 8), (5, 0)))
    _is(E, 2, chunk4=True)
    _vs_oracle(E, ref)
    _same(E, D, bitwise=False)
    G = _run(ns, nlob, n, np_, (), gray_only=True)
    _is(G, 0, streams=inr)
    refg = _ref(O, G, ("gray", ns))
    _vs_oracle(G, refg)
    H = _run(ns, nlob, n, np_, ((5, 0),), gray_only=True)
    _is(H, 0)
    _vs_oracle(H, refg)
    _same(G, H, bitwise=not inr)


def _batch(O, ns, nlob, np_, Bs, cia=False):
    """Column.run_batch of B = Bs[0] columns (and the first Bs[1:] of them) on the short grid: band fluxes of three columns against the
    oracle and against single-column runs, and of the smaller batch against the larger"""
    cs = clearsky_jl_amd
    n = N_SHORT
    ctx = cs.Context(0)
    try:
        col = _column(ns, nlob, n, np_, ctx, cia)
        T0 = W.earth_temperature(col.P)
        B = Bs[0]
        Ts = [T0 + (b / B) * np.linspace(-4.0, 6.0, len(T0)) for b in range(B)]
        Fu, Fd = col.run_batch(Ts)
        assert not col.work()["dispatch"]["flags"] & RT_STREAMS
        for B2 in Bs[1:]:
            Fu2, Fd2 = col.run_batch(Ts[:B2])
            assert not col.work()["dispatch"]["flags"] & RT_STREAMS
            fm = Fu[:B2].max()
            assert np.max(np.abs(Fu2 - Fu[:B2])) < 1e-13 * fm and np.max(np.abs(Fd2 - Fd[:B2])) < 1e-13 * fm
        for b in (0, B // 2, B - 1):
            col.update(Ts[b])
            col.run()
            Fs = col.fetch()
            fm = Fs[0].max()
            assert np.max(np.abs(Fu[b] - Fs[0])) < 1e-13 * fm and np.max(np.abs(Fd[b] - Fs[1])) < 1e-13 * fm
            ref = _oracle(O, col, want_sigma=False)
            fm = ref["Fup"].max()
            tol = 1e-10 if cia else 1e-11
            assert np.max(np.abs(Fu[b] - ref["Fup"])) < tol * fm and np.max(np.abs(Fd[b] - ref["Fdn"])) < tol * fm
    finally:
        ctx.close()


@pytest.mark.parametrize("ns", range(1, 17))
def test_stream_sweep_batch(O, ns):
    """k_rt<NS, false> (one wave per tile): a batch whose tiles x B reaches 4096 waves; B one below runs k_rt<NS, true>"""
    t = _tiles(N_SHORT)
    B = -(-4096 // t)
    assert not _ud(N_SHORT, B) and _ud(N_SHORT, B - 1)
    _batch(O, ns, 2, 7, (B, B - 1))


@pytest.mark.parametrize("ns", range(2, 9))
def test_scan_per_rule(O, ns):
    """k_flux_scan<NS, 5> up to five layers per wave (nl = 60 over 12 waves), <NS, 0> from six (nl = 61) and for NS 7, 8; key 15 | 2048
    forces <NS, 0>: bitwise either way (test_scan_transmissivities_in_registers_equal_recomputed)"""
    n = N_SHORT
    np5 = _first_n(lambda q: _scan_per(q) > 5, 20, 200)
    for np_ in (np5 - 1, np5):
        assert _scan_sh(np_, 2, ns) <= LIM and (_scan_per(np_) <= 5) == (np_ < np5)
        a = _run(ns, 2, n, np_)
        b = _run(ns, 2, n, np_, ((15, 2048),))
        _is(a, 3)
        _is(b, 3)
        _vs_oracle(a, _ref(O, a, ("per", ns, np_)))
        _same(b, a, bitwise=True)
    assert np5 - 1 == 61


# ---- b. every Lobatto order ----------------------------------------------------------------------------------------------------

LAYERS = {2: 9, 3: 7, 4: 10, 5: 6, 6: 8, 7: 5, 8: 7, 9: 6, 10: 9, 11: 4, 12: 6, 13: 5, 14: 7, 15: 5, 16: 6}
DENSE = (7, 12)          # the near-line plane (sigma2) live: key 7 = 2
CIA = (5, 13)            # a CIA pair, added per 16-state load in the chunk form


def test_lobatto_sweep_covers_the_chunk_loads():
    """K mod 16 takes many values over the sweep; every order whose nlob - 1 does not divide 16 has a layer whose nodes come from two of
    the chunk form's 16-state loads"""
    Ks = {nlob: _K(nl + 1, nlob) for nlob, nl in LAYERS.items()}
    assert len({K % 16 for K in Ks.values()}) >= 8
    for nlob, nl in LAYERS.items():
        d = nlob - 1
        straddle = any(i * d < 16 * m < (i + 1) * d for i in range(nl) for m in range(1, Ks[nlob] // 16 + 1))
        assert straddle == (16 % d != 0), nlob


@pytest.mark.parametrize("nlob", range(2, 17))
def test_lobatto_sweep(O, nlob):
    """NS = 4: the scan form (default), k_flux_chunk3 (keys 15 = 2, 5 = 0), k_rt<4, true> (key 15 = 1, key 5 = 0) against the oracle and each
    other; the batch k_rt<4, false>"""
    n, ns, np_ = N_SHORT, 4, LAYERS[nlob] + 1
    cia = nlob in CIA
    base = ((7, 2),) if nlob in DENSE else ()
    assert _scan_sh(np_, nlob, ns) <= LIM and _chunk_sh(np_, nlob) <= LIM and _scan_per(np_) <= 5
    R = _run(ns, nlob, n, np_, base + ((15, 1), (5, 0)), cia)
    _is(R, 0)
    ref = _ref(O, R, ("lob", nlob))
    _vs_oracle(R, ref)
    S = _run(ns, nlob, n, np_, base, cia)
    _is(S, 3)
    _vs_oracle(S, ref)
    _same(S, R, bitwise=False)
    Ch = _run(ns, nlob, n, np_, base + ((15, 2), (5, 0)), cia)
    _is(Ch, 2)
    _vs_oracle(Ch, ref)
    _same(Ch, R, bitwise=not cia)
    if base:
        for r in (R, S, Ch):
            assert r["streams"] & 2, r["streams"]
    t = _tiles(n)
    _batch(O, ns, nlob, np_, (-(-4096 // t),), cia)


# ---- c. the LDS limits ---------------------------------------------------------------------------------------------------------

def test_scan_lds_limit(O):
    """the scan form up to ~156 KB of LDS (K + 2 np - 1 + 2 (NS + 1) rows of 64): at nlobatto 2, NS 5 crossed near 100 levels; past it
    form 0 with k_rt_streams (its own LDS still fits).  Below: against k_rt_streams (key 15 = 1); past: against k_rt<5, true> (key 5 = 0)"""
    n, ns, nlob = N_SHORT, 5, 2
    npx = _first_n(lambda q: _scan_sh(q, nlob, ns) > LIM, 20, 400)
    assert 95 <= npx <= 105 and _rt_streams(n, npx, ns)
    b = _run(ns, nlob, n, npx - 1)
    _is(b, 3)
    _vs_oracle(b, _ref(O, b, ("scanlds", npx - 1)))
    _same(_run(ns, nlob, n, npx - 1, ((15, 1),)), b, bitwise=False)
    a = _run(ns, nlob, n, npx)
    _is(a, 0, streams=True)
    _vs_oracle(a, _ref(O, a, ("scanlds", npx)))
    f = _run(ns, nlob, n, npx, ((5, 0),))
    _is(f, 0)
    _same(f, a, bitwise=False)


def test_rt_streams_lds_limit(O):
    """k_rt_streams<8> up to ~156 KB of LDS (2 np - 1 + 4 NS rows of 64): a tall column on each side (key 15 = 1: the separate
    kernels); below against k_rt<8, true> (key 5 = 0), past it k_rt<8, true> runs"""
    n, ns, nlob = N_SHORT, 8, 2
    npx = _first_n(lambda q: _streams_sh(q, ns) > LIM, 20, 1000)
    assert _rt_streams(n, npx - 1, ns) and not _rt_streams(n, npx, ns)
    b = _run(ns, nlob, n, npx - 1, ((15, 1),))
    _is(b, 0, streams=True)
    _vs_oracle(b, _ref(O, b, ("rtlds", npx - 1)))
    _same(_run(ns, nlob, n, npx - 1, ((15, 1), (5, 0))), b, bitwise=False)
    a = _run(ns, nlob, n, npx, ((15, 1),))
    _is(a, 0)
    _vs_oracle(a, _ref(O, a, ("rtlds", npx)))


def test_chunk_lds_limit(O):
    """the chunk form up to ~156 KB of LDS (2 np x 4 band-sum slots + 4 waves x R = 16 + nlob - 1 ring rows of 64): at nlobatto 2 a
    column of ~1950 levels on a 65-point grid (two tiles, the last of one point; CO2 lines within 5 cm^-1), key 15 = 2; below against the
    separate kernels (bitwise), past it form 0"""
    n, ns, nlob, cut = 65, 4, 2, 5.0
    npx = _first_n(lambda q: _chunk_sh(q, nlob) > LIM, 20, 5000)
    assert _K(npx, nlob) <= 65535
    b = _run(ns, nlob, n, npx - 1, ((15, 2),), cut=cut)
    _is(b, 2)
    _vs_oracle(b, _ref(O, b, ("chunklds", npx - 1)))
    _same(b, _run(ns, nlob, n, npx - 1, ((15, 1), (5, 0)), cut=cut), bitwise=True)
    a = _run(ns, nlob, n, npx, ((15, 2),), cut=cut)
    _is(a, 0)
    _vs_oracle(a, _ref(O, a, ("chunklds", npx)))


# ---- d. entry points -----------------------------------------------------------------------------------------------------------

def test_fluxes_discretized_16_16(O):
    """cs_fluxes_discretized, marshalled like the Julia ccall, at Discretized(16, 16): 8 layers, K = 121"""
    cs = clearsky_jl_amd
    ctx = cs.Context(0)
    try:
        col = _column(16, 16, N_SHORT, 9, ctx, _setup=False)
        r = _julia_call(cs, ctx, col.nu, col.P, col.g, 16, col.Tn, col.mun, col.Tlev, [_lines("CO2")], ["voigt"], [25.0], col.conc,
                        col.sigma_gray, None, col.S_toa, col.albedo, THETA_S, 16)
    finally:
        ctx.close()
    ref = _oracle(O, col, want_sigma=False)
    assert relerr(r["tau"], ref["tau"]) < 1e-11
    sm = max(ref["Mup"].max(), ref["Mdn"].max())
    amp = source_rounding_bound(cs, col.nu, col.Tlev, ref["tau"])
    for k in ("Mup", "Mdn"):
        assert np.max(np.abs(r[k] - ref[k])) < 1e-11 * sm + amp, k
    for k in ("Fup", "Fdn"):
        assert np.max(np.abs(r[k] - ref[k])) < 1e-11 * ref["Fup"].max(), k


@pytest.mark.parametrize("ns,nlob", [(0, 2), (17, 2), (4, 1), (4, 17)])
def test_orders_outside_the_abi_refused(ns, nlob):
    """cs_column_setup (through Column), cs_fluxes_discretized and cs_fluxes_discretized_members refuse nstream 0 / 17 and nlobatto
    1 / 17 with CS_EINVAL (before they read the node arrays, which are those of a valid column here)"""
    cs = clearsky_jl_amd
    ctx = cs.Context(0)
    try:
        col = _column(4, 2, 640, 5, ctx, _setup=False)
        col.core = cs.Discretized(ns, nlob)
        with pytest.raises(cs.ClearSkyHIPError) as e:
            col._setup()
        assert e.value.code == CS_EINVAL
        with pytest.raises(cs.ClearSkyHIPError) as e:
            _julia_call(cs, ctx, col.nu, col.P, col.g, nlob, col.Tn, col.mun, col.Tlev, [_lines("CO2")], ["voigt"], [25.0], col.conc,
                        col.sigma_gray, None, col.S_toa, col.albedo, THETA_S, ns)
        assert e.value.code == CS_EINVAL
        colc = _column(4, 2, 640, 5, ctx, cia=True, _setup=False)
        colc.core = cs.Discretized(ns, nlob)
        with pytest.raises(cs.ClearSkyHIPError) as e:
            cs.core._fluxes_discretized(colc, None, None, None)        # (a CIA pair among the members: cs_fluxes_discretized_members)
        assert e.value.code == CS_EINVAL
        col.core = cs.Discretized(4, 2)                                # (the context is still usable)
        col._setup()
        col.run()
        assert np.all(np.isfinite(col.fetch()[0])) and col.info()["flux_form"] == 3
    finally:
        ctx.close()
