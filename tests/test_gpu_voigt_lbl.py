"""Shape code 7, LBLRTM's line calculation at pressure-shifted centres (include/clearsky_hip.h, CS_SHAPE_VOIGT_LBL), on the device through
every entry point that takes a shape.

Expected values come from tests/voigt_lbl_ref.py: per distinct shift s, the oracle's code-6 parts of the lines sharing it -- the direct,
pedestal-removed sum on the grid nu - s and the mirror sum on nu + s -- added over s, times R at the true nu; test_voigt_lbl.py holds
that restatement to 40-digit values and checks the premises of the cases here (membership by shifted centre differing from membership
by table position on both sides of every edge, reversed neighbours, exactness).  Errors are taken against R times the sum of the
magnitudes of the parts, the sum BEFORE the pedestal is subtracted (ckdvvh_ref.err), at every point: no probe is left out.

Bars.  Exact shifts (delta a multiple of 2^-5, nul of 2^-6, P a dyadic multiple of P0, dyadic grids: nul + s, nu - c and nu + c are
exact in fp64): 1e-11, the bar tests/test_gpu_voigt_ckdvvh.py holds code 6 to.  Arbitrary pressures (the golden file's own delta; the
node pressures of a column): the device rounds delta P / P0 and nul + s, |dc| <= U (|c| + 2 |s|), which a Doppler core of width
alpha = 3e-6 nul turns into ~1e-10 of the value -- the centre term of lineparam_bound; those comparisons use the 1e-9 that
tests/test_gpu_pressure_shift.py uses for the same reason.  Device against device: 5e-13."""
import ctypes as C
import os

import numpy as np
import pytest

import ckdvvh_ref as X
import voigt_lbl_ref as V
import workloads as W
from conftest import HITRAN, relerr
from test_gpu_pressure_shift import write_par

pytestmark = pytest.mark.gpu

CUT = 25.0
KATM = V.KATM
EINVAL = -1
PSHIFT = 16


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("lbl"))


@pytest.fixture(scope="module")
def ctx(cs):
    c = cs.Context(0)
    yield c
    c.close()


def _par(cs, tmp, name, t, da=None):
    return cs.SpectralLines(write_par(os.path.join(tmp, name + ".par"), 1, t["nu"], t["S"], t["gamma_a"], t["gamma_s"], t["Epp"], t["na"],
                                      t["delta_a"] if da is None else da))


@pytest.fixture(scope="module")
def case(cs, tmp):
    """the exact-shift table (voigt_lbl_ref.case_table) through a .par file"""
    return _par(cs, tmp, "case", V.case_table())


@pytest.fixture(scope="module")
def h2o_low(cs):
    return cs.SpectralLines(os.path.join(HITRAN, "H2O.par"), numin=0.0, numax=150.0)


@pytest.mark.parametrize("cut", [25.0, 5.0, 1.0, 0.25])
def test_b1_exact_shifts_and_edges(cs, O, ctx, case, cut):
    """The low grid (two tiles, one ragged, nu_1 < D) and the edge grid (nu_1 - D among the lines), nine states (an octet and a tail, P
    from 0 to 2 P0): vector method (strict pre-filter on each state's shifted centres) and scalar method (none) against the reference.
    cut = 0.25 lies below the largest shift (0.375): no line is certainly inside, the whole window is tested state by state."""
    T, P, Pp = V.states()
    da = case.delta_a
    differs = False
    for name, nu in (("low", V.GRID), ("edge", V.EDGE_GRID)):
        sv = cs.shape_batch(case, "voigtLBL", nu, T, P, Pp, cut, ctx)
        sp = cs.shape_points(case, "voigtLBL", nu, T, P, Pp, cut, ctx)
        s6 = cs.shape_batch(case, "voigtCKDVVH", nu, T, P, Pp, cut, ctx)
        for k in range(len(T)):
            for s, strict in ((sv[k], True), (sp[k], False)):
                assert np.all(np.isfinite(s)) and np.all(s >= 0)
                ref = V.expected(cs, O, case, da, nu, T[k], P[k], Pp[k], cut, strict)
                e = X.err(s, ref)
                print(f"cut {cut} {name} state {k} strict {strict}: {e:.2e}")
                assert e < 1e-11, (name, k, strict, e)
            differs = differs or not np.array_equal(sv[k], sp[k])
            if P[k] == 0.0:     # no shift at P = 0: code 6, on the code-6 scale
                assert X.err(sv[k], X.expected(cs, O, case, nu, T[k], P[k], Pp[k], cut, True)) < 1e-11
            elif P[k] >= 0.25 * KATM and cut == 25.0:   # the shift is no rounding matter
                assert np.mean(np.abs(sv[k] - s6[k]) > 1e-6 * s6[k]) > 0.5, k
    assert differs   # (the pre-filter dropped a line at some state that the scalar method kept)
    if cut == 25.0:     # the in-place and scalar-nu forms
        nu = V.GRID
        sv = cs.shape_batch(case, "voigtLBL", nu, T[4:5], P[4:5], Pp[4:5], cut, ctx)[0]
        sp = cs.shape_points(case, "voigtLBL", nu, T[4:5], P[4:5], Pp[4:5], cut, ctx)[0]
        s = np.zeros_like(nu)
        assert cs.voigtLBL_(s, nu, case, T[4], P[4], Pp[4], ctx=ctx) is None
        assert np.array_equal(s, sv) and np.array_equal(cs.voigtLBL(nu, case, T[4], P[4], Pp[4], ctx=ctx), sv)
        assert cs.voigtLBL(float(nu[77]), case, T[4], P[4], Pp[4], ctx=ctx) == sp[77]


def test_zero_shift_is_code_6(cs, O, ctx, tmp):
    """a file with every delta = 0: the code-6 expected values, and the device's own code 6"""
    t = V.case_table()
    zero = _par(cs, tmp, "zero", t, np.zeros(len(t["nu"])))
    assert np.all(zero.delta_a == 0)
    T, P, Pp = V.states()
    nu = V.GRID
    s7 = cs.shape_batch(zero, "voigtLBL", nu, T, P, Pp, CUT, ctx)
    p7 = cs.shape_points(zero, "voigtLBL", nu, T, P, Pp, CUT, ctx)
    s6 = cs.shape_batch(zero, "voigtCKDVVH", nu, T, P, Pp, CUT, ctx)
    for k in range(len(T)):
        ref = X.expected(cs, O, zero, nu, T[k], P[k], Pp[k], CUT, True)
        assert X.err(s7[k], ref) < 1e-11, k
        assert X.err(p7[k], X.expected(cs, O, zero, nu, T[k], P[k], Pp[k], CUT, False)) < 1e-11, k
        z = ref[1] == 0.0   # (no line reaches the point, e.g. the Doppler cores of the P = 0 state: both are exact zeros)
        assert np.array_equal(s7[k][z], s6[k][z]) and np.max(np.abs(s7[k][~z] - s6[k][~z]) / ref[1][~z]) < 5e-13, k


def test_file_shifts_b1(cs, O, ctx, h2o_low):
    """the golden H2O file's own delta_a at arbitrary pressures (1e-9: the module docstring)"""
    sl = h2o_low
    assert np.mean(sl.delta_a != 0) > 0.5
    nu = np.unique(np.concatenate([[0.0, 1e-3], np.linspace(0.01, 110.0, 2001)]))
    T, P, Pp = [230.0, 290.0, 251.3], [87654.3, 3123.4, 151987.5], [1234.5, 10.0, 40.0]
    sv = cs.shape_batch(sl, "voigtLBL", nu, T, P, Pp, CUT, ctx)
    sp = cs.shape_points(sl, "voigtLBL", nu, T, P, Pp, CUT, ctx)
    for k in range(len(T)):
        for s, strict in ((sv[k], True), (sp[k], False)):
            assert s[0] == 0.0 and np.all(s >= 0) and np.all(np.isfinite(s))
            e = X.err(s, V.expected(cs, O, sl, sl.delta_a, nu, T[k], P[k], Pp[k], CUT, strict))
            print(f"file shifts state {k} strict {strict}: {e:.2e}")
            assert e < 1e-9, (k, strict, e)


# ---- columns ----------------------------------------------------------------------------------------------------------------------

def _sample(n):
    """first and last tile whole, 64 points in between"""
    last = n - ((n - 1) % 64 + 1)
    mid = np.random.default_rng(n).choice(np.arange(64, last), 64, replace=False)
    return np.unique(np.concatenate([np.arange(64), mid, np.arange(last, n)]))


def _column(cs, ctx, gases, npl, nlob, nstream=5, **kw):
    P = cs.pressuregrid(10.0, 1e5, npl)
    return cs.Column(P, 9.8, W.earth_temperature(P), 0.029, 0.0, 0.0, *gases, core=cs.Discretized(nstream, nlob), ctx=ctx, **kw)


def _fetch(col):
    col.run()
    tau = np.zeros((col.nl, col.nnu), order="F")
    Mu = np.zeros((col.np, col.nnu), order="F")
    Md = np.zeros((col.np, col.nnu), order="F")
    Fup, Fdn = col.fetch(tau, Mu, Md)
    return dict(tau=tau, Mup=Mu, Mdn=Md, Fup=Fup, Fdn=Fdn)


def node_extra(cs, O, col, gi, x):
    """(C_k sigma_7, C_k scale) of column gas gi at the points x and every node state (the scalar method's lines: no pre-filter)"""
    g = col.gases[gi]
    out, mag = np.zeros((col.K, len(x))), np.zeros((col.K, len(x)))
    for k in range(col.K):
        Ck = col.conc[gi, k]
        v, m = V.expected(cs, O, g.sl, g.sl.delta_a, x, col.Tk[k], col.Pk[k], Ck * col.Pk[k], g.dnu_cut, False)
        out[k], mag[k] = Ck * v, Ck * m
    return out, mag


# every flux form the step dispatches, picked by grid size as tests/test_gpu_voigt_ckdvvh.py picks them: tiles, cs_set_tuning, flux_form
FORMS = [(300, {15: 1}, 0), (600, {}, 3), (600, {15: 1}, 0), (2000, {}, 0), (4200, {}, 2), (4200, {15: 1}, 0)]


@pytest.mark.parametrize("tiles,tune,form", FORMS, ids=[f"{t}tiles-{f}{'-unfused' if u else ''}" for t, u, f in FORMS])
def test_column_flux_forms(cs, O, lines, case, tiles, tune, form):
    """the case table as code 7 beside CO2 as code 0 on 0.5 .. 120 cm^-1 (mirror terms in the first 25): sigma at the nodes against the
    reference, fluxes against the oracle column of CO2 with C x sigma_7 as sigma_extra (node pressures are arbitrary: 1e-9)"""
    n = 64 * tiles
    nu = np.linspace(0.5, 120.0, n)
    c = cs.Context(0)
    for k_, v in tune.items():
        c.set_tuning(k_, v)
    gases = [cs.DirectGas(case, W.fC_h2o, nu, shape="voigtLBL"), cs.DirectGas(lines("CO2"), 400e-6, nu)]
    col = _column(cs, c, gases, 9, 2)
    r = _fetch(col)
    assert col.info()["flux_form"] == form, col.info()
    assert col.info()["groups"] == 2
    whole = n <= 20000
    idx = np.arange(n) if whole else _sample(n)
    extra, mag = node_extra(cs, O, col, 0, nu[idx])
    ref = O.fluxes_discretized(nu[idx], col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [col.gases[1].sl], ["voigt"], [CUT], col.conc[1:],
                               sigma_extra=extra, theta_s=col.theta_s, nstream=col.core.nstream, want_sigma=True)
    sig = col.sigma_nodes()[:, idx]
    assert np.max(np.abs(sig - ref["sigma"]) / np.maximum(mag + ref["sigma"], 1e-300)) < 1e-9
    assert relerr(r["tau"][:, idx], ref["tau"]) < 1e-9
    sm = max(ref["Mup"].max(), ref["Mdn"].max())
    for k in ("Mup", "Mdn"):
        assert np.max(np.abs(r[k][:, idx] - ref[k])) < 1e-9 * sm, k
    if whole:
        for k in ("Fup", "Fdn"):
            assert np.max(np.abs(r[k] - ref[k])) < 1e-9 * np.max(ref["Fup"]), k
    c.close()


@pytest.mark.parametrize("npl,nlob,K", [(4, 3, 7), (5, 5, 17)], ids=["K7", "K17"])
def test_column_entry_points(cs, O, lines, case, npl, nlob, K):
    """(np, nlobatto) = (4, 3) and (5, 5): the node planes of cs_column_run against B1 at the node states and against the reference;
    cs_column_sigma_run's clamp; cs_column_update_state far from the first profile; cs_column_batch against sequential runs;
    cs_accel_store; two nu-shards adding up; cs_column_counts by shifted centre; run-to-run and graph-replay bitwise identity"""
    n = 6000
    nu = np.linspace(0.5, 120.0, n)
    c = cs.Context(0)
    gases = [cs.DirectGas(case, W.fC_h2o, nu, shape="voigtLBL"), cs.DirectGas(lines("CO2"), 400e-6, nu)]
    col = _column(cs, c, gases, npl, nlob, 3)
    assert col.K == K
    r1 = _fetch(col)
    sig = col.sigma_nodes()
    r2 = _fetch(col)
    for k in r1:
        assert np.array_equal(r1[k], r2[k]), k
    idx = _sample(n)
    extra, mag = node_extra(cs, O, col, 0, nu[idx])
    co2 = np.array([col.conc[1, k] * cs.shape_points(lines("CO2"), "voigt", nu[idx], [col.Tk[k]], [col.Pk[k]], [col.conc[1, k] * col.Pk[k]], CUT, c)[0]
                    for k in range(K)])
    assert np.max(np.abs(sig[:, idx] - extra - co2) / np.maximum(mag + co2, 1e-300)) < 1e-9
    # B1 at the node states (device against device: the same records, the column's windows against the call's)
    for k in (0, K // 2, K - 1):
        Ck = col.conc[0, k]
        b1 = Ck * cs.shape_points(case, "voigtLBL", nu, [col.Tk[k]], [col.Pk[k]], [Ck * col.Pk[k]], CUT, c)[0]
        s5 = Ck * cs.shape_points(case, "voigtVVH", nu, [col.Tk[k]], [col.Pk[k]], [Ck * col.Pk[k]], CUT, c)[0]
        full = b1 + col.conc[1, k] * cs.shape_points(lines("CO2"), "voigt", nu, [col.Tk[k]], [col.Pk[k]], [col.conc[1, k] * col.Pk[k]], CUT, c)[0]
        assert np.max(np.abs(sig[k] - full) / np.maximum(s5 + full, 1e-300)) < 5e-13, k
    # the clamp of the total plane, and the counts by shifted centre
    col.sigma_run()
    s_run = col.sigma_nodes()
    assert np.all(s_run >= 0) and np.max(np.abs(s_run - np.maximum(sig, 0.0))) <= 5e-13 * np.max(sig)
    cnt = col.counts()
    def inside(centres):   # (as the library counts: lines in [nu - cut, nu + cut] of the sorted centres)
        cc = np.sort(centres)
        return int(np.sum(np.searchsorted(cc, nu + CUT, "right") - np.searchsorted(cc, nu - CUT, "left")))
    pairs = sum(inside(case.nu + case.delta_a * col.Pk[k] / KATM) for k in range(K))
    assert pairs != inside(case.nu) * K            # (by shifted centre, state by state: not the table positions')
    co2_pairs = inside(lines("CO2").nu) * K
    assert cnt["pair_evals"] == pairs + co2_pairs, (cnt, pairs, co2_pairs)
    # update_state far from the first profile, against a fresh column at that profile
    T2 = np.array(col.Tlev)[::-1] + 11.0
    col.update(T2)
    u = _fetch(col)
    fresh = cs.Column(col.P, 9.8, cs.AtmosphericProfile(col.P, T2), 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, nlob), ctx=c)
    f = _fetch(fresh)
    for k in u:
        assert np.max(np.abs(u[k] - f[k])) <= 5e-13 * np.max(np.abs(f[k])), k
    # cs_column_batch against sequential runs
    Tlev = np.array(fresh.Tlev)
    Ts = [Tlev] + [Tlev + 1.0 * (np.arange(npl) == i) for i in range(0, npl, 2)]
    bcol = cs.Column(col.P, 9.8, cs.AtmosphericProfile(col.P, Tlev), 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, nlob), ctx=c, want_tau=False,
                     want_M=False)
    Bu, Bd = bcol.run_batch(Ts, 0.029)
    for b, Tb in enumerate(Ts):
        one = cs.Column(col.P, 9.8, cs.AtmosphericProfile(col.P, Tb), 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, nlob), ctx=c, want_tau=False,
                        want_M=False)
        one.run()
        Fu, Fd = one.fetch()
        assert np.max(np.abs(Bu[b] - Fu)) < 5e-13 * np.max(Fu) and np.max(np.abs(Bd[b] - Fd)) < 5e-13 * np.max(Fu)
    # cs_accel_store over a code-7 column (clamped: every log finite) = the column's sigma at the knots
    Pe = cs.pressuregrid(10.0, 1e5, 6)
    Te = np.clip(W.earth_temperature(Pe), 160.0, 340.0)
    A = cs.AcceleratedAbsorber(Te, Pe, *gases, ctx=c)
    kcol = A._knots
    kcol.sigma_run()
    s = kcol.sigma_nodes()
    assert np.all(s >= 0)
    kn = np.zeros((len(Pe), n))
    cs.check(cs.lib().cs_accel_fetch(c.handle, A.slot, n, len(Pe), cs.dptr(kn)))
    ls = np.log(np.maximum(s, np.finfo(float).tiny))
    assert np.all(np.isfinite(kn)) and np.max(np.abs(kn - ls)) < 1e-14 * np.max(np.abs(ls))
    # two nu-ranges (the first holds the mirror terms; lines shift across the boundary's reach) add up to the whole
    P = col.P
    T = W.earth_temperature(P)
    F = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, nlob), ctx=c)
    Fu = 0.0
    for rg in ((0, 2500), (2500, n)):
        part = cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, nlob), ctx=c, nu_range=rg)
        part.run()
        Fu = Fu + part.fetch()[0]
    assert np.max(np.abs(Fu - F.Fup)) < 1e-12 * np.max(F.Fup)
    mc = cs.MultiContext([0, 0])
    G = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, nlob), ctx=mc)
    assert np.max(np.abs(G.Fup - F.Fup)) < 1e-12 * np.max(F.Fup)
    mc.close()
    c.close()
    # graph replay: eager, capture, replay, replay
    g = cs.Context(0)
    g.set_tuning(4, 1)
    gcol = _column(cs, g, gases, npl, nlob, 3)
    outs = [_fetch(gcol) for _ in range(4)]
    for k in r1:
        assert np.max(np.abs(outs[0][k] - r1[k])) <= 5e-13 * np.max(np.abs(r1[k])), k
        for o in outs[1:]:
            assert np.array_equal(o[k], outs[0][k]), k
    g.close()


def test_bake(cs, O, ctx, case):
    """a 5 x 7 cs_bake: the knots are ln of B1 (vector method, per-state pre-filter) at the knot states"""
    nu = V.GRID
    Om = cs.AtmosphericDomain((200.0, 320.0), 5, (0.125 * KATM, 2.0 * KATM), 7)
    g = cs.Gas(case, 0.01, nu, Om, shape="voigtLBL", ctx=ctx, keep_host_tables=True)
    Z = g.lnsigma
    assert Z.shape == (len(nu), 5, 7) and not np.any(np.isnan(Z))
    TT, PP = np.meshgrid(Om.T, Om.P, indexing="ij")
    Tf, Pf = TT.ravel(order="F"), PP.ravel(order="F")
    s = cs.shape_batch(case, "voigtLBL", nu, Tf, Pf, 0.01 * Pf, CUT, ctx)
    for q in range(0, len(Tf), 6):   # the knot values themselves (arbitrary pressures: 1e-9)
        assert X.err(s[q], V.expected(cs, O, case, case.delta_a, nu, Tf[q], Pf[q], 0.01 * Pf[q], CUT, True)) < 1e-9, q
    flat = s.T.reshape(len(nu), Om.nT, Om.nP, order="F")
    tiny = np.finfo(float).tiny
    with np.errstate(divide="ignore"):
        ref = np.where(np.all(flat <= tiny, axis=(1, 2))[:, None, None], np.log(tiny), np.log(flat))
    assert np.array_equal(np.isfinite(Z), np.isfinite(ref))
    m = np.isfinite(ref) & (ref > np.log(tiny))
    assert np.max(np.abs(Z[m] - ref[m])) < 1e-12 * np.max(np.abs(ref[m]))


def test_refusals_and_merging(cs, lines, case):
    """through the C ABI: code 7 runs on a slot loaded from a file, is refused on one filled by cs_gas_upload (never a shift of zero),
    takes no flag and no other bit; code 7 merges only with code 7 of the same cut-off"""
    c = cs.Context(0)
    L = cs.lib()
    sl = lines("CO2")
    slot = c.slot_of(sl, shift=True)
    nu = np.linspace(600.0, 700.0, 101)
    T, P, Pp = np.array([296.0]), np.array([KATM]), np.array([40.0])
    out = np.zeros(len(nu))

    def call(code, slot_=slot, fn=L.cs_shape_batch):
        return fn(c.handle, slot_, code, CUT, len(nu), cs.dptr(nu), 1, cs.dptr(T), cs.dptr(P), cs.dptr(Pp), cs.dptr(out), len(nu))
    assert call(7) == 0 and call(7, fn=L.cs_shape_points) == 0
    for code in (7 | PSHIFT, 7 | 32, 8, 15, 23, 6 | PSHIFT):
        assert call(code) == EINVAL, code
    par = {k: getattr(sl, k) for k in ("nu", "S", "gamma_a", "gamma_s", "Epp", "na")}
    bare = cs.SpectralLines(dict(M=np.full(len(sl.nu), 2, np.int16), I=sl.I, A=np.zeros(len(sl.nu)), **par))
    s2 = c.slot_of(bare)
    assert call(7, s2) == EINVAL and call(7, s2, L.cs_shape_points) == EINVAL and call(6, s2) == 0
    with pytest.raises(ValueError):   # (refused in Python first, with the reason)
        cs.shape_batch(bare, "voigtLBL", nu, T, P, Pp, CUT, c)
    # a re-upload through cs_gas_upload drops the shifts: code 7 is refused from then on
    arrs = [cs.as_f64(a) for a in (sl.nu, sl.S, sl.gamma_a, sl.gamma_s, sl.Epp, sl.na, sl.mu)]
    iso = np.ascontiguousarray(sl.I, dtype=np.int16)
    ncheb = np.ascontiguousarray(sl.ncheb, dtype=np.int32)
    cheb = cs.as_f64(sl.cheb)
    assert L.cs_gas_upload(c.handle, slot, len(arrs[0]), *[cs.dptr(a) for a in arrs], iso.ctypes.data_as(C.POINTER(C.c_int16)),
                           len(ncheb), ncheb.ctypes.data_as(C.POINTER(C.c_int32)), cs.dptr(cheb)) == 0
    assert call(7) == EINVAL and call(6) == 0
    c.close()
    # merging, by Column.info()'s groups and Column.work()
    c = cs.Context(0)
    g = np.linspace(0.5, 120.0, 4000)
    h2o = cs.SpectralLines(os.path.join(HITRAN, "H2O.par"), numin=0.0, numax=150.0)

    def col_of(*gs):
        col = _column(cs, c, list(gs), 4, 3, 3)
        col.sigma_run()
        return col, col.sigma_nodes()
    a = cs.DirectGas(case, W.fC_h2o, g, shape="voigtLBL")
    col, s_a = col_of(a)
    w = col.work()   # (a code-7 group takes no matrix-core pieces)
    assert w["edge_mx_flops_useful"] == 0 and w["node_evals_matrix"] == 0 and w["nodes_mx_flops_useful"] == 0, w
    for b, ngroups in ((cs.DirectGas(h2o, 1e-3, g, shape="voigtLBL"), 1), (cs.DirectGas(h2o, 1e-3, g, shape="voigtLBL", dnu_cut=20.0), 2),
                       (cs.DirectGas(h2o, 1e-3, g, shape="voigtCKDVVH"), 2), (cs.DirectGas(h2o, 1e-3, g, pressure_shift=True), 2)):
        col, s_ab = col_of(b, a)
        assert col.info()["groups"] == ngroups, (b.shape, b.dnu_cut, col.info())
        s_b = col_of(b)[1]
        nop = col_of(cs.DirectGas(case, W.fC_h2o, g, shape="voigtVVH"), cs.DirectGas(h2o, 1e-3, g, shape="voigtVVH"))[1]
        assert np.max(np.abs(s_ab - np.maximum(s_a + s_b, 0.0)) / np.maximum(nop, 1e-300)) < 5e-13, (b.shape, b.dnu_cut)
    c.close()
