"""Shape code 6, the pedestal-removed Van Vleck-Huber Voigt (include/clearsky_hip.h, CS_SHAPE_VOIGT_CKD_VVH), on the device through every
entry point that takes a shape.

Expected values come from tests/ckdvvh_ref.py: the oracle's Voigt of the S~-scaled table, minus per-line pedestals, plus the mirror terms
minus theirs, times R(nu, T) -- the pedestals and mirror terms from a vectorised restatement that test_voigt_ckdvvh.py checks against
one-line oracle slices and 40-digit arithmetic.  B1 errors are taken against R times the sum of the magnitudes of the parts, since the
pedestal difference cancels near every cut-off.  Columns compare against the oracle column of the other gases with sigma_extra =
C x sigma_6 at every node.  Tolerances are the suite's: 1e-11 against the oracle, 5e-13 device against device, 2e-13 interpolation on
against off.
"""
import os

import numpy as np
import pytest

import ckdvvh_ref as X
import workloads as W
from clearsky_jl_amd import DISPATCH_FLAGS
from conftest import HITRAN, relerr

pytestmark = pytest.mark.gpu

CUT = X.CUT
STATES = [(220.0, 50.0, 0.02), (296.0, 101325.0, 40.53), (260.0, 3e3, 30.0)]
RT_STREAMS = DISPATCH_FLAGS["RT_STREAMS"]   # Column.work()["dispatch"]["flags"]


@pytest.fixture(scope="module")
def ctx(cs):
    c = cs.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def h2o_low(cs):
    """the golden H2O lines below 150 cm^-1: 13 below the cut-off, the lowest at 8.4e-5 cm^-1"""
    return cs.SpectralLines(os.path.join(HITRAN, "H2O.par"), numin=0.0, numax=150.0)


def test_b1_vector_and_scalar(cs, O, ctx, h2o_low):
    nu = np.unique(np.concatenate([[0.0, 1e-6, 1e-3], np.linspace(0.01, 110.0, 6001), CUT - h2o_low.nu[:13]]))
    T, P, Pp = map(list, zip(*STATES))
    sv = cs.shape_batch(h2o_low, "voigtCKDVVH", nu, T, P, Pp, CUT, ctx)
    sp = cs.shape_points(h2o_low, "voigtCKDVVH", nu, T, P, Pp, CUT, ctx)
    s5 = cs.shape_batch(h2o_low, "voigtVVH", nu, T, P, Pp, CUT, ctx)
    for k in range(len(T)):
        for s, strict in ((sv[k], True), (sp[k], False)):
            assert np.all(np.isfinite(s)) and np.all(s >= 0)
            assert s[0] == 0.0                                   # nu = 0
            assert X.err(s, X.expected(cs, O, h2o_low, nu, T[k], P[k], Pp[k], strict=strict)) < 1e-11, (k, strict)
        # the pedestals are real: far from line centres they are most of the code-5 value
        m = s5[k] > 0
        assert np.max((s5[k][m] - sv[k][m]) / s5[k][m]) > 0.5
    s = np.zeros_like(nu)
    assert cs.voigtCKDVVH_(s, nu, h2o_low, T[1], P[1], Pp[1], ctx=ctx) is None
    assert np.array_equal(s, sv[1])
    assert np.array_equal(cs.voigtCKDVVH(nu, h2o_low, T[1], P[1], Pp[1], ctx=ctx), sv[1])
    assert cs.voigtCKDVVH(float(nu[777]), h2o_low, T[1], P[1], Pp[1], ctx=ctx) == sp[1][777]


def _one(cs, sl, l):
    return cs.SpectralLines(dict(M=np.full(1, 1, np.int16), I=sl.I[l:l + 1], nu=sl.nu[l:l + 1], S=sl.S[l:l + 1],
                                 gamma_a=sl.gamma_a[l:l + 1], gamma_s=sl.gamma_s[l:l + 1], Epp=sl.Epp[l:l + 1], na=sl.na[l:l + 1],
                                 A=np.zeros(1), delta_a=np.zeros(1)))


def test_cutoff_and_mirror_edges_one_line(cs, O, ctx, h2o_low):
    """One line: inclusive ends at nul +- cut and at the mirror edge cut - nul; sigma_6 -> 0 from inside at nul +- cut; no jump at the
    mirror edge beyond rounding, where code 5 jumps by R S~ f(cut)"""
    T, P, Pp = STATES[1]
    d = np.array([1e-1, 1e-3])
    for target in (10.0, 100.0):
        l = int(np.argmin(np.abs(h2o_low.nu - target)))
        one = _one(cs, h2o_low, l)
        nl = one.nu[0]
        edges = [nl + CUT, CUT - nl, nl - CUT]
        nu = np.concatenate([np.linspace(0.0, nl + 40.0, 801), *[[e, e - dd, e + dd] for e in edges for dd in d]])
        nu = np.unique(nu[nu >= 0.0])
        pc = X.line_terms(cs, O, one, [CUT], T, P, Pp, [0])[0]
        for s, strict in ((cs.shape_batch(one, "voigtCKDVVH", nu, [T], [P], [Pp], CUT, ctx)[0], True),
                          (cs.shape_points(one, "voigtCKDVVH", nu, [T], [P], [Pp], CUT, ctx)[0], False)):
            assert X.err(s, X.expected(cs, O, one, nu, T, P, Pp, strict=strict)) < 1e-11, (target, strict)
            assert np.all(s >= 0)
            out = (np.abs(nu - nl) > CUT) & (nu + nl > CUT)
            assert np.all(s[out] == 0.0)
            for e in (nl + CUT, nl - CUT):   # the direct edges: inclusive (the term is there, and is rounding), -> 0 from inside
                if e <= 0.0:
                    continue
                i = np.nonzero(nu == e)[0][0]
                assert s[i] <= 1e-13 * X.R(cs, e, T) * pc
                for dd in d:
                    inner = s[np.nonzero(nu == (e - dd if e > nl else e + dd))[0][0]]
                    assert 0.0 < inner < 2.0 * X.R(cs, e, T) * pc * 2.0 * dd / CUT, (e, dd)
            if nl < CUT:
                e = CUT - nl
                i = np.nonzero(nu == e)[0][0]
                j = np.nonzero(nu == e + d[1])[0][0]
                step = X.R(cs, e, T) * pc
                # continuous: over d[1] the profile moves by ~1e-2 of the step (the direct term's slope), not by a step
                assert abs(s[i] - s[j]) < 0.05 * step, (s[i] - s[j], step)
                s5 = cs.shape_batch(one, "voigtVVH", nu, [T], [P], [Pp], CUT, ctx)[0] if strict else \
                    cs.shape_points(one, "voigtVVH", nu, [T], [P], [Pp], CUT, ctx)[0]
                # code 5 steps there by R S~ f(cut): code 5 - code 6 is R S~ f(cut) x (the number of terms present), 2 at i and 1 at j
                jump = (s5[i] - s[i]) - (s5[j] - s[j])
                assert abs(jump - step) < 1e-3 * step, (jump, step)
                assert s5[i] - s5[j] > 0.9 * step


# The synthetic table of the bench workload (a line every 0.05 cm^-1 from 0 to 2525) at the bench grid's spacing, from 0.5 cm^-1: some
# 500 lines reach the mirror term, and the grid is dense enough for every matrix-core piece
NU0, DNU = 0.5, 0.008


def _syn_nu(n):
    return NU0 + DNU * np.arange(n)


def _sample(n):
    """first and last tile whole, 64 points in between"""
    last = n - ((n - 1) % 64 + 1)
    mid = np.random.default_rng(n).choice(np.arange(64, last), 64, replace=False)
    return np.unique(np.concatenate([np.arange(64), mid, np.arange(last, n)]))


def _column(cs, ctx, gases, P, T, **kw):
    return cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=ctx, **kw)


def _fetch(col):
    col.run()
    tau = np.zeros((col.nl, col.nnu), order="F")
    Mu = np.zeros((col.np, col.nnu), order="F")
    Md = np.zeros((col.np, col.nnu), order="F")
    Fup, Fdn = col.fetch(tau, Mu, Md)
    return dict(tau=tau, Mup=Mu, Mdn=Md, Fup=Fup, Fdn=Fdn)


def node_extra(cs, O, col, gi, x):
    """C_k sigma_6 of column gas gi at the points x and every node state (the inclusive-cut-off scalar method's lines)"""
    g = col.gases[gi]
    out = np.zeros((col.K, len(x)))
    for k in range(col.K):
        Ck = col.conc[gi, k]
        out[k] = Ck * X.expected(cs, O, g.sl, x, col.Tk[k], col.Pk[k], Ck * col.Pk[k], strict=False)[0]
    return out


def _vs_oracle(col, r, ref, whole):
    assert relerr(r["tau"], ref["tau"]) < 1e-11
    sm = max(ref["Mup"].max(), ref["Mdn"].max())
    for k in ("Mup", "Mdn"):
        assert np.max(np.abs(r[k] - ref[k])) < 1e-11 * sm, k
    if whole:
        for k in ("Fup", "Fdn"):
            assert np.max(np.abs(r[k] - ref[k])) < 1e-11 * np.max(ref["Fup"]), k


def test_b1_long_grid_interp_on_off(cs, O):
    sl = W.lines("synthetic", "H2O")
    n = 100000
    nu = _syn_nu(n)
    T = list(np.linspace(200.0, 310.0, 20))
    P = list(np.geomspace(30.0, 1e5, 20))
    Pp = [0.01 * p for p in P]
    res = {}
    for on in (True, False):
        c = cs.Context(0)
        c.set_interp(on)
        res[on] = cs.shape_batch(sl, "voigtCKDVVH", nu, T, P, Pp, CUT, c)
        c.close()
    assert np.all(res[True] >= 0) and np.all(np.isfinite(res[True])) and np.all(res[False] >= 0)
    c = cs.Context(0)
    s5 = cs.shape_batch(sl, "voigtVVH", nu, T, P, Pp, CUT, c)
    c.close()
    assert np.max(np.abs(res[True] - res[False]) / np.maximum(s5, 1e-300)) < 2e-13   # (on the code-5 scale: the pedestal cancels)
    idx = _sample(n)
    x = nu[idx]
    assert x[0] == nu[0] and x[-1] == nu[-1]   # (so the strict pre-filter is that of the whole grid)
    for k in range(0, 20, 3):
        ref = X.expected(cs, O, sl, x, T[k], P[k], Pp[k])
        for on in (True, False):
            assert X.err(res[on][k][idx], ref) < 1e-11, (k, on)


def test_matrix_core_forms_interp_on_off(cs, O):
    """A code-6 column (synthetic H2O, K = 61) on a 2000-tile grid from 0.5 cm^-1: with interpolation on, the interpolated far wings,
    the matrix-core node sums and the window ends on the matrix cores run, as Column.work() reports; with it off, none of them"""
    sl = W.lines("synthetic", "H2O")
    n = 64 * 2000
    nu = _syn_nu(n)
    P = cs.pressuregrid(10.0, 1e5, 61)
    T = W.earth_temperature(P)
    res = {}
    for on in (True, False):
        ctx = cs.Context(0)
        ctx.set_interp(on)
        col = _column(cs, ctx, [cs.DirectGas(sl, W.fC_h2o, nu, shape="voigtCKDVVH")], P, T)
        assert col.K == 61
        r = _fetch(col)
        r["sigma"], r["work"], r["col"] = col.sigma_nodes(), col.work(), col
        res[on] = r
        w = r["work"]
        if on:
            assert w["levels"] > 0 and w["node_evals"] > 0, w
            assert w["node_evals_matrix"] > 0 and w["nodes_mx_flops_useful"] > 0, w    # k_cheb_nodes_mx
            assert w["edge_mx_flops_useful"] > 0, w                                      # k_voigt_edge_mx
        else:
            assert w["levels"] == 0 and w["node_evals"] == 0 and w["node_evals_matrix"] == 0 and w["edge_mx_flops_useful"] == 0, w
        ctx.close()
    a, b = res[True], res[False]
    assert np.all(np.isfinite(a["sigma"]))
    col = a["col"]
    idx = _sample(n)
    extra = node_extra(cs, O, col, 0, nu[idx])
    scale = np.max(np.abs(extra), axis=1, keepdims=True)
    assert np.max(np.abs(a["sigma"] - b["sigma"]) / np.max(np.abs(a["sigma"]), axis=1, keepdims=True)) < 2e-13
    assert relerr(a["tau"], b["tau"]) < 2e-13
    ref = O.fluxes_discretized(nu[idx], col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [], [], [], np.zeros((0, col.K)), sigma_extra=extra,
                               theta_s=col.theta_s, nstream=col.core.nstream, want_sigma=True)
    for r in (a, b):
        assert np.max(np.abs(r["sigma"][:, idx] - ref["sigma"]) / scale) < 1e-11
        _vs_oracle(col, {k: r[k][:, idx] for k in ("tau", "Mup", "Mdn")}, ref, False)


# every flux form the step dispatches, picked by grid size (test_gpu_dispatch): tiles, cs_set_tuning, expected (flux_form, k_rt_streams)
FORMS = [(300, {15: 1}, 0, True), (600, {}, 3, False), (600, {15: 1}, 0, False), (2000, {}, 0, False), (4200, {}, 2, False),
         (4200, {15: 1}, 0, False)]


@pytest.mark.parametrize("tiles,tune,form,streams", FORMS, ids=[f"{t}tiles-{f}{'-streams' if s else ''}{'-unfused' if u else ''}"
                                                               for t, u, f, s in FORMS])
def test_column_flux_forms(cs, O, lines, h2o_low, tiles, tune, form, streams):
    """H2O as code 6 beside CO2 as code 0 on 0.5 .. 120 cm^-1 (mirror terms in the first 25): the oracle column of CO2 with
    C x sigma_6 of H2O as sigma_extra"""
    n = 64 * tiles
    nu = np.linspace(0.5, 120.0, n)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    for k_, v in tune.items():
        ctx.set_tuning(k_, v)
    gases = [cs.DirectGas(h2o_low, W.fC_h2o, nu, shape="voigtCKDVVH"), cs.DirectGas(lines("CO2"), 400e-6, nu)]
    col = _column(cs, ctx, gases, P, T)
    r = _fetch(col)
    assert col.info()["flux_form"] == form, col.info()
    assert bool(col.work()["dispatch"]["flags"] & RT_STREAMS) == streams, col.work()["dispatch"]
    whole = n <= 20000
    idx = np.arange(n) if whole else _sample(n)
    ref = O.fluxes_discretized(nu[idx], col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [col.gases[1].sl], ["voigt"], [CUT], col.conc[1:],
                               sigma_extra=node_extra(cs, O, col, 0, nu[idx]), theta_s=col.theta_s, nstream=col.core.nstream)
    _vs_oracle(col, {k: (r[k][:, idx] if k in ("tau", "Mup", "Mdn") else r[k]) for k in r}, ref, whole)
    ctx.close()


def test_merge_groups_and_repeat(cs, lines, h2o_low):
    """code 6 never merges with codes 0, 4 or 5, and merges with code 6 of the same cut-off; a column of codes 0, 4, 5 and 6 equals the
    sum of its single-group parts; a repeated run is bitwise the same; a sigma_run plane with a code-6 group holds no negative.  Sums
    are compared on the scale of the same gases without pedestals (codes 4 -> 0, 6 -> 5), since the pedestal difference cancels"""
    nu = np.linspace(0.5, 300.0, 8000)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    nopd = {"voigtCKD": "voigt", "voigtCKDVVH": "voigtVVH"}

    def h2o(shape):
        return cs.DirectGas(h2o_low, W.fC_h2o, nu, shape=shape)

    def co2(shape, cut=CUT):
        return cs.DirectGas(lines("CO2"), 400e-6, nu, shape=shape, dnu_cut=cut)

    def sig(gs):
        c = _column(cs, ctx, gs, P, T)
        c.sigma_run()
        return c.sigma_nodes(), c

    def scale(gs):
        return sig([cs.DirectGas(g.sl, g.fC, nu, shape=nopd.get(g.shape, g.shape), dnu_cut=g.dnu_cut) for g in gs])[0]
    a = h2o("voigtCKDVVH")
    s_a, _ = sig([a])
    assert np.all(s_a >= 0)
    for b, ngroups in ((co2("voigt"), 2), (co2("voigtCKD"), 2), (co2("voigtVVH"), 2), (co2("voigtCKDVVH"), 1),
                       (co2("voigtCKDVVH", 20.0), 2)):
        s_ab, c = sig([b, a])
        assert c.info()["groups"] == ngroups, (b.shape, c.info())
        assert np.all(s_ab >= 0)
        s_b, _ = sig([b])
        assert np.max(np.abs(s_ab - (s_a + s_b)) / np.maximum(scale([b, a]), 1e-300)) < 5e-13, (b.shape, b.dnu_cut)
        c.sigma_run()
        assert np.array_equal(c.sigma_nodes(), s_ab)
    # codes 0, 4, 5 and 6 in one column (four groups): the sum of the parts, and bitwise repeatable through the flux step
    parts = [co2("voigt"), h2o("voigtCKD"), h2o("voigtVVH"), a]
    s_all, c = sig(parts)
    assert c.info()["groups"] == 4
    tot = sum(sig([g])[0] for g in parts)
    assert np.max(np.abs(s_all - tot) / np.maximum(scale(parts), 1e-300)) < 5e-13
    col = _column(cs, ctx, parts, P, T)
    r1, r2 = _fetch(col), _fetch(col)
    for k in ("tau", "Mup", "Mdn", "Fup", "Fdn"):
        assert np.array_equal(r1[k], r2[k]), k
    ctx.close()


def test_bake(cs, O, h2o_low):
    """Mode T: the knots are ln sigma_6 at the knot states (empty rows at ln floatmin), and a column over the baked gas follows them"""
    ctx = cs.Context(0)
    nu = np.linspace(0.5, 100.0, 3000)
    Om = cs.AtmosphericDomain((150.0, 350.0), 12, (10.0, 1e5), 24)
    g = cs.Gas(h2o_low, 0.01, nu, Om, shape="voigtCKDVVH", ctx=ctx, keep_host_tables=True)
    Z = g.lnsigma
    assert not np.any(np.isnan(Z))
    TT, PP = np.meshgrid(Om.T, Om.P, indexing="ij")
    Tf, Pf = TT.ravel(order="F"), PP.ravel(order="F")
    s = cs.shape_batch(h2o_low, "voigtCKDVVH", nu, Tf, Pf, 0.01 * Pf, CUT, ctx)
    for q in range(0, len(Tf), 37):   # the knot values themselves against the expected values
        assert X.err(s[q], X.expected(cs, O, h2o_low, nu, Tf[q], Pf[q], 0.01 * Pf[q])) < 1e-11, q
    # ln of them as the code-4 bake takes it: a row that is empty everywhere at ln floatmin, zeros in a row that is not at -inf
    flat = s.T.reshape(len(nu), Om.nT, Om.nP, order="F")
    tiny = np.finfo(float).tiny
    with np.errstate(divide="ignore"):
        ref = np.where(np.all(flat <= tiny, axis=(1, 2))[:, None, None], np.log(tiny), np.log(flat))
    assert np.array_equal(np.isfinite(Z), np.isfinite(ref))
    m = np.isfinite(ref) & (ref > np.log(tiny))
    assert np.max(np.abs(Z[m] - ref[m])) < 1e-12 * np.max(np.abs(ref[m]))
    P = cs.pressuregrid(20.0, 9e4, 7)
    T = np.clip(W.earth_temperature(P), 160.0, 340.0)
    col = _column(cs, ctx, [g], P, T)
    col.sigma_run()
    sig = col.sigma_nodes()
    assert np.all(sig >= 0)
    for k in range(col.K):
        assert relerr(sig[k], 0.01 * O.table_sigma(Z, Om.T, Om.P, col.Tk[k], col.Pk[k]), floor=1e-300) < 1e-11
    ctx.close()


def test_batch_accel_shards(cs, lines, h2o_low):
    nu = np.linspace(0.5, 120.0, 6000)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    gases = [cs.DirectGas(h2o_low, W.fC_h2o, nu, shape="voigtCKDVVH"), cs.DirectGas(lines("CO2"), 400e-6, nu)]
    # cs_column_batch of the np+1 jacobian! profiles against sequential runs
    col = _column(cs, ctx, gases, P, T, want_tau=False, want_M=False)
    Tlev = np.array(col.Tlev)
    Ts = [Tlev] + [Tlev + 1.0 * (np.arange(len(P)) == i) for i in range(len(P))]
    Bu, Bd = col.run_batch(Ts, 0.029)
    for b, Tb in enumerate(Ts):
        one = _column(cs, ctx, gases, P, cs.AtmosphericProfile(P, Tb), want_tau=False, want_M=False)
        one.run()
        Fu, Fd = one.fetch()
        assert np.max(np.abs(Bu[b] - Fu)) < 5e-13 * np.max(Fu) and np.max(np.abs(Bd[b] - Fd)) < 5e-13 * np.max(Fu)
    # cs_accel_store over a code-6 column (clamped: no negative, every log finite) = sigma_fetch of that column at the knots
    Pe = cs.pressuregrid(10.0, 1e5, 12)
    Te = np.clip(W.earth_temperature(Pe), 160.0, 340.0)
    A = cs.AcceleratedAbsorber(Te, Pe, *gases, ctx=ctx)
    kcol = A._knots
    kcol.sigma_run()
    s = kcol.sigma_nodes()
    assert np.all(s >= 0)
    kn = np.zeros((len(Pe), len(nu)))
    cs.check(cs.lib().cs_accel_fetch(ctx.handle, A.slot, len(nu), len(Pe), cs.dptr(kn)))
    assert np.all(np.isfinite(kn))
    ls = np.log(np.maximum(s, np.finfo(float).tiny))
    assert np.max(np.abs(kn - ls)) < 1e-14 * np.max(np.abs(ls))
    # two nu-ranges (the first holds the mirror terms, the second starts above the cut-off: direct pedestals and R only) add up to
    # the whole
    F = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=ctx)
    assert nu[2500] > CUT
    parts = [cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=ctx, nu_range=r) for r in ((0, 2500), (2500, 6000))]
    Fu = 0.0
    for c in parts:
        c.run()
        Fu = Fu + c.fetch()[0]
    assert np.max(np.abs(Fu - F.Fup)) < 1e-12 * np.max(F.Fup)
    ctx.close()
