"""Shape code 4, the pedestal-removed Voigt of the MT_CKD convention (include/clearsky_hip.h, CS_SHAPE_VOIGT_CKD), on the device
through every entry point that takes a shape.

The oracle knows only the reference's four shapes, so the expected values are assembled here from pieces checked on their own:
  sigma_ckd(nu) = max(0, voigt(nu) - sum_{l in window(nu)} p_l),   p_l = the oracle's Voigt of the ONE-line slice l at nul + cut
(with inclusive semantics), the window being the lines voigt itself includes.  Columns compare against the oracle column of the
gas as "voigt" with sigma_extra = -(concentration x pedestal sum) at every node.

Tolerances are those of the Voigt tests of the same path (test_gpu_parity, test_gpu_merge, test_gpu_interp); B1 errors are taken
relative to max|sigma| of the restatement, because the pedestal difference cancels near each line's cut-off.
"""
import numpy as np
import pytest

import workloads as W
from conftest import HITRAN, relerr

pytestmark = pytest.mark.gpu

STATES = [(220.0, 50.0, 0.02), (296.0, 101325.0, 40.53), (260.0, 3e3, 30.0)]
CUT = 25.0


@pytest.fixture(scope="module")
def ctx(cs):
    c = cs.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def h2o(cs):
    """a few hundred H2O lines of the golden .par (the one-line restatement loops over them)"""
    return cs.SpectralLines(HITRAN + "/H2O.par", numin=1500.0, numax=1700.0)


class _Slice:
    pass


def _slice(sl, a, b):
    o = _Slice()
    for n in ("nu", "S", "gamma_a", "gamma_s", "Epp", "na", "mu", "I"):
        setattr(o, n, np.ascontiguousarray(getattr(sl, n)[a:b]))
    o.ncheb, o.cheb = sl.ncheb, sl.cheb
    return o


def pedestals(O, sl, T, P, Pp, cut):
    """p_l = S_l fvoigt(cut; alpha_l, gamma_l) of every line: the oracle's Voigt of the one-line slice at nul + cut (its cut-off
    doubled so that the rounding of nul + cut cannot drop the line; the profile moves by ~1e-14 over that rounding)"""
    return np.array([O.shape_bang("voigt", [sl.nu[l] + cut], _slice(sl, l, l + 1), T, P, Pp, 2.0 * cut, strict_ends=False)[0]
                     for l in range(len(sl.nu))])


def windows(nul, x, cut):
    """[j0, j1) per point: the lines with |x - nul| <= cut, by the line kernels' own test"""
    L = len(nul)
    j0 = np.searchsorted(nul, x - cut, "left")
    j1 = np.searchsorted(nul, x + cut, "right")
    for _ in range(3):   # settle the rounding at the two ends onto the exact predicate
        m = (j0 > 0) & ~(x - nul[np.maximum(j0 - 1, 0)] > cut); j0[m] -= 1
        m = (j0 < L) & (x - nul[np.minimum(j0, L - 1)] > cut); j0[m] += 1
        m = (j1 > 0) & (nul[np.maximum(j1 - 1, 0)] - x > cut); j1[m] -= 1
        m = (j1 < L) & ~(nul[np.minimum(j1, L - 1)] - x > cut); j1[m] += 1
    return j0, np.maximum(j1, j0)


def pedestal_sum(nul, p, x, cut, strict):
    """sum of p over each point's window (strict: the vector method's end-point pre-filter first), in extended precision"""
    keep = (nul > x[0] - cut) & (nul < x[-1] + cut) if strict else np.ones(len(nul), bool)
    g0 = int(np.argmax(keep)) if keep.any() else 0
    g1 = g0 + int(keep.sum())
    j0, j1 = windows(nul[g0:g1], x, cut)
    c = np.concatenate([[0.0], np.cumsum(p[g0:g1].astype(np.longdouble))])
    return (c[j1] - c[j0]).astype(float)


def restate(O, sl, nu, T, P, Pp, cut=CUT, strict=True):
    v = O.shape_bang("voigt", nu, sl, T, P, Pp, cut, strict_ends=strict)
    return np.maximum(v - pedestal_sum(sl.nu, pedestals(O, sl, T, P, Pp, cut), nu, cut, strict), 0.0)


def node_pedestal(O, col, gi, cut=CUT):
    """-(C_k x pedestal sum) of column gas gi at every node: the oracle column's sigma_extra"""
    g = col.gases[gi]
    out = np.zeros((col.K, col.nnu))
    for k in range(col.K):
        Ck = col.conc[gi, k]
        p = pedestals(O, g.sl, col.Tk[k], col.Pk[k], Ck * col.Pk[k], cut)
        out[k] = -Ck * pedestal_sum(g.sl.nu, p, col.nu, cut, False)
    return out


def test_b1_vector_and_scalar(cs, O, ctx, h2o):
    nu = np.linspace(1480.0, 1720.0, 5003)
    T, P, Pp = map(list, zip(*STATES))
    sv = cs.shape_batch(h2o, "voigtCKD", nu, T, P, Pp, CUT, ctx)
    sp = cs.shape_points(h2o, "voigtCKD", nu, T, P, Pp, CUT, ctx)
    for k in range(len(T)):
        rv = restate(O, h2o, nu, T[k], P[k], Pp[k], strict=True)
        rp = restate(O, h2o, nu, T[k], P[k], Pp[k], strict=False)
        assert np.all(sv[k] >= 0) and np.all(sp[k] >= 0)
        assert np.max(np.abs(sv[k] - rv)) < 5e-12 * np.max(rv)
        assert np.max(np.abs(sp[k] - rp)) < 5e-12 * np.max(rp)
        # the pedestal is real: far from line centres it is most of the Voigt value
        v = cs.shape_batch(h2o, "voigt", nu, [T[k]], [P[k]], [Pp[k]], CUT, ctx)[0]
        assert np.max((v - sv[k]) / v) > 0.5
    # the in-place and scalar wrappers
    s = np.zeros_like(nu)
    assert cs.voigtCKD_(s, nu, h2o, T[1], P[1], Pp[1], ctx=ctx) is None
    assert np.array_equal(s, sv[1])
    assert np.array_equal(cs.voigtCKD(nu, h2o, T[1], P[1], Pp[1], ctx=ctx), sv[1])
    assert cs.voigtCKD(float(nu[777]), h2o, T[1], P[1], Pp[1], ctx=ctx) == sp[1][777]


def test_cutoff_one_line(cs, O, ctx, h2o):
    l = int(np.argmax(h2o.S))
    one = cs.SpectralLines(dict(M=np.full(1, 1, np.int16), I=h2o.I[l:l + 1], nu=h2o.nu[l:l + 1], S=h2o.S[l:l + 1],
                                gamma_a=h2o.gamma_a[l:l + 1], gamma_s=h2o.gamma_s[l:l + 1], Epp=h2o.Epp[l:l + 1], na=h2o.na[l:l + 1],
                                A=np.zeros(1), delta_a=np.zeros(1)))
    nl = one.nu[0]
    d = np.array([1e-1, 1e-2, 1e-3])
    nu = np.sort(np.concatenate([nl + np.linspace(-40.0, 40.0, 801), [nl - CUT, nl + CUT], nl - CUT + d, nl + CUT - d,
                                 nl - CUT - d, nl + CUT + d]))
    nu = np.unique(nu)
    T, P, Pp = STATES[1]
    for s in (cs.shape_batch(one, "voigtCKD", nu, [T], [P], [Pp], CUT, ctx)[0], cs.shape_points(one, "voigtCKD", nu, [T], [P], [Pp], CUT, ctx)[0]):
        assert np.all(s >= 0)
        assert np.all(s[np.abs(nu - nl) > CUT] == 0.0)                   # beyond the cut: exactly zero
        peak = s.max()
        edge = s[np.abs(np.abs(nu - nl) - CUT) < 1e-9]
        assert np.all(edge <= 1e-15 * peak)                              # at the cut: the pedestal cancels the line to rounding
        p = pedestals(O, one, T, P, Pp, CUT)[0]
        for dd in d:   # continuous at the cut: delta inside it, sigma = p (2 delta / cut) to first order (a far wing ~ 1/dnu^2)
            inner = s[np.abs(np.abs(nu - nl) - (CUT - dd)) < 1e-9]
            assert len(inner) == 2 and np.all(np.abs(inner / (p * 2.0 * dd / CUT) - 1.0) < 0.02), (dd, inner, p)
    # vector and scalar methods agree on a grid whose ends lie within the cut of lines outside it
    nu = np.linspace(1560.0, 1600.0, 2001)
    a = cs.shape_batch(h2o, "voigtCKD", nu, [T], [P], [Pp], CUT, ctx)[0]
    b = cs.shape_points(h2o, "voigtCKD", nu, [T], [P], [Pp], CUT, ctx)[0]
    assert np.max(np.abs(a - b)) < 1e-13 * np.max(b)


def pedestals_vec(cs, O, sl, T, P, Pp, cut, lines=None):
    """the same p_l for many lines at once: S_l(T), alpha_l(T), gamma_l(T, P, Pp) written out as scaleintensity / alphadoppler /
    gammalorentz (line_shapes.jl:107-123, 144, 255-257), the profile as fvoigt (:366-378) with the oracle's Re w.  Checked against
    the one-line slices in test_pedestals_vectorised."""
    C_ = cs.constants
    j = np.arange(len(sl.nu)) if lines is None else np.asarray(lines)
    nul, E, I = sl.nu[j], sl.Epp[j], sl.I[j]
    c2 = 100.0 * C_.h * C_.c / C_.k
    qr = np.array([O.chebyQrefQ(T, sl.cheb[i][: sl.ncheb[i]]) if sl.ncheb[i] > 0 else np.nan for i in range(len(sl.ncheb))])
    S = sl.S[j] * qr[I - 1] * (np.exp(-c2 * E / T) * (1.0 - np.exp(-c2 * nul / T))) / (np.exp(-c2 * E / C_.Tref) * (1.0 - np.exp(-c2 * nul / C_.Tref)))
    alpha = (nul / C_.c) * np.sqrt(2.0 * C_.R * T / sl.mu[j])
    gamma = (C_.Tref / T) ** sl.na[j] * (sl.gamma_a[j] * (P - Pp) + sl.gamma_s[j] * Pp) / C_.atm
    d = np.sqrt(np.log(2.0)) / alpha
    return S * np.sqrt(np.log(2.0) / np.pi) / alpha * O.faddeeva(cut * d, gamma * d)


def test_pedestals_vectorised(cs, O, h2o):
    for T, P, Pp in STATES:
        assert relerr(pedestals_vec(cs, O, h2o, T, P, Pp, CUT), pedestals(O, h2o, T, P, Pp, CUT)) < 1e-12


# The synthetic tables of the bench workload (test_gpu_dispatch: 40 lines per cm^-1 together) on its grid spacing: dense enough for
# the window ends on the matrix cores (edge_in_use: 4 lines per 64-point tile) and, with K = 61 node states, for the matrix-core node
# sums of the interpolated far wings
NU0, DNU = 300.0, 0.008


def _syn_nu(n):
    return NU0 + DNU * np.arange(n)


def _sample(n):
    """first and last tile whole, 64 points in between (test_gpu_dispatch._vs_oracle)"""
    last = n - ((n - 1) % 64 + 1)
    mid = np.random.default_rng(n).choice(np.arange(64, last), 64, replace=False)
    return np.unique(np.concatenate([np.arange(64), mid, np.arange(last, n)]))


def test_b1_long_grid_interp_on_off(cs, O):
    """B1 over 20 states on a 1e5-point grid of the dense synthetic H2O table: interpolated far wings on and off agree at the long-grid
    Voigt fuzz's bar (test_gpu_fuzz: 2e-13), and both match the restatement at the B1 bar on a sample of the grid (its two end points
    included, so the strict end-point pre-filter is the same)"""
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
        res[on] = cs.shape_batch(sl, "voigtCKD", nu, T, P, Pp, CUT, c)
        c.close()
    assert np.all(res[True] >= 0) and np.all(res[False] >= 0)
    assert relerr(res[True], res[False], floor=1e-280) < 2e-13
    idx = _sample(n)
    lines = np.nonzero((sl.nu > nu[0] - CUT) & (sl.nu < nu[-1] + CUT))[0]
    for k in range(0, 20, 3):
        p = np.zeros(len(sl.nu))
        p[lines] = pedestals_vec(cs, O, sl, T[k], P[k], Pp[k], CUT, lines)
        r = np.maximum(O.shape_bang("voigt", nu[idx], sl, T[k], P[k], Pp[k], CUT) - pedestal_sum(sl.nu, p, nu[idx], CUT, True), 0.0)
        for on in (True, False):
            assert np.max(np.abs(res[on][k][idx] - r)) < 5e-12 * np.max(r), (k, on)


def test_matrix_core_forms_interp_on_off(cs, O):
    """A code-4 column (synthetic H2O, K = 61) on a 2000-tile grid: with interpolation on, the interpolated far wings, the matrix-core
    node sums (k_cheb_nodes_mx) and the window ends on the matrix cores (k_voigt_edge_mx) are what runs, as Column.work() reports;
    with it off, none of them.  Both against the oracle column (gas as "voigt", the pedestal as sigma_extra) at the suite's bar, and
    against each other at the long-grid fuzz's"""
    sl = W.lines("synthetic", "H2O")
    n = 64 * 2000
    nu = _syn_nu(n)
    P = cs.pressuregrid(10.0, 1e5, 61)
    T = W.earth_temperature(P)
    res = {}
    for on in (True, False):
        ctx = cs.Context(0)
        ctx.set_interp(on)
        col = _column(cs, ctx, [cs.DirectGas(sl, W.fC_h2o, nu, shape="voigtCKD")], P, T)
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
    assert np.all(a["sigma"] >= 0) and np.all(b["sigma"] >= 0)
    assert relerr(a["sigma"], b["sigma"], floor=1e-280) < 2e-13 and relerr(a["tau"], b["tau"]) < 2e-13
    col = a["col"]
    idx = _sample(n)
    lines = np.nonzero((sl.nu >= nu[0] - 2 * CUT) & (sl.nu <= nu[-1] + 2 * CUT))[0]
    extra = np.zeros((col.K, len(idx)))
    for k in range(col.K):
        Ck = col.conc[0, k]
        p = np.zeros(len(sl.nu))
        p[lines] = pedestals_vec(cs, O, sl, col.Tk[k], col.Pk[k], Ck * col.Pk[k], CUT, lines)
        extra[k] = -Ck * pedestal_sum(sl.nu, p, nu[idx], CUT, False)
    ref = O.fluxes_discretized(nu[idx], col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [sl], ["voigt"], [CUT], col.conc, sigma_extra=extra,
                               theta_s=col.theta_s, nstream=col.core.nstream, want_sigma=True)
    for r in (a, b):
        assert relerr(r["sigma"][:, idx], np.maximum(ref["sigma"], 0.0), floor=1e-280) < 1e-11
        assert relerr(r["tau"][:, idx], ref["tau"]) < 1e-11
        sm = max(ref["Mup"].max(), ref["Mdn"].max())
        for k in ("Mup", "Mdn"):
            assert np.max(np.abs(r[k][:, idx] - ref[k])) < 1e-11 * sm, k


def _column(cs, ctx, gases, P, T, **kw):
    return cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=ctx, **kw)


def _fetch(col):
    col.run()
    tau = np.zeros((col.nl, col.nnu), order="F")
    Mu = np.zeros((col.np, col.nnu), order="F")
    Md = np.zeros((col.np, col.nnu), order="F")
    Fup, Fdn = col.fetch(tau, Mu, Md)
    return dict(tau=tau, Mup=Mu, Mdn=Md, Fup=Fup, Fdn=Fdn)


@pytest.mark.parametrize("nnu,form", [(20000, "fused"), (270000, "chunk")])
def test_column_vs_oracle(cs, O, lines, h2o, nnu, form):
    """H2O as code 4 beside CO2 as Voigt: the oracle column of both as Voigt with the H2O pedestal passed as sigma_extra"""
    nu = np.linspace(1520.0, 1680.0, nnu)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    gases = [cs.DirectGas(h2o, W.fC_h2o, nu, shape="voigtCKD"), cs.DirectGas(lines("CO2"), 400e-6, nu)]
    col = _column(cs, ctx, gases, P, T)
    r = _fetch(col)
    info = col.info()
    assert info["flux_form"] in ((1, 3) if form == "fused" else (2,)), info
    extra = node_pedestal(O, col, 0)
    ref = O.fluxes_discretized(col.nu, col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [g.sl for g in col.gases], ["voigt", "voigt"],
                               [CUT, CUT], col.conc, sigma_extra=extra, theta_s=col.theta_s, nstream=col.core.nstream)
    assert relerr(r["tau"], ref["tau"]) < 1e-11
    sm = np.max(ref["Mup"])
    for k in ("Mup", "Mdn"):
        assert np.max(np.abs(r[k] - ref[k])) < 1e-11 * sm, k
    for k in ("Fup", "Fdn"):
        assert np.max(np.abs(r[k] - ref[k])) < 1e-11 * np.max(ref["Fup"]), k
    ctx.close()


def test_merge_never_mixes_code_0_and_4(cs, lines, h2o):
    """a code-0 and a code-4 gas of the same cut in one column: the sum of the two one-gas columns, through sigma_fetch"""
    nu = np.linspace(1500.0, 1700.0, 8000)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    a = cs.DirectGas(h2o, W.fC_h2o, nu, shape="voigtCKD")
    b = cs.DirectGas(lines("CH4"), 1.8e-6, nu)
    both = _column(cs, ctx, [a, b], P, T)
    both.sigma_run()
    s_ab = both.sigma_nodes()
    assert both.info()["groups"] == 2
    sa = _column(cs, ctx, [a], P, T)
    sa.sigma_run()
    s_a = sa.sigma_nodes()
    sb = _column(cs, ctx, [b], P, T)
    sb.sigma_run()
    s_b = sb.sigma_nodes()
    assert np.all(s_a >= 0)
    assert relerr(s_ab, s_a + s_b, floor=1e-300) < 5e-13
    ctx.close()


def test_bake(cs, O, h2o):
    """Mode T: the knots are ln of shape_batch code 4 at the knot states (no NaN), and a column over the baked gas follows them"""
    ctx = cs.Context(0)
    nu = np.linspace(1500.0, 1700.0, 3000)
    Om = cs.AtmosphericDomain((150.0, 350.0), 12, (10.0, 1e5), 24)
    g = cs.Gas(h2o, 0.01, nu, Om, shape="voigtCKD", ctx=ctx, keep_host_tables=True)
    Z = g.lnsigma
    assert not np.any(np.isnan(Z))
    TT, PP = np.meshgrid(Om.T, Om.P, indexing="ij")
    s = cs.shape_batch(h2o, "voigtCKD", nu, TT.ravel(order="F"), PP.ravel(order="F"), 0.01 * PP.ravel(order="F"), CUT, ctx)
    flat = s.T.reshape(len(nu), Om.nT, Om.nP, order="F")
    tiny = np.finfo(float).tiny
    z = (flat.reshape(len(nu), -1).min(axis=1) == 0) & (flat.reshape(len(nu), -1).max(axis=1) > 0)
    flat[z] = 0.0
    with np.errstate(divide="ignore"):
        ref = np.where(np.all(flat <= tiny, axis=(1, 2))[:, None, None], np.log(tiny), np.log(flat))
    assert np.array_equal(np.isfinite(Z), np.isfinite(ref))
    m = np.isfinite(ref) & (ref > np.log(tiny))
    assert np.max(np.abs(Z[m] - ref[m])) < 1e-12 * np.max(np.abs(ref[m]))
    # a column over the baked gas against the table interpolant at its nodes
    P = cs.pressuregrid(20.0, 9e4, 7)
    T = np.clip(W.earth_temperature(P), 160.0, 340.0)
    col = _column(cs, ctx, [g], P, T)
    col.sigma_run()
    sig = col.sigma_nodes()
    for k in range(col.K):
        assert relerr(sig[k], 0.01 * O.table_sigma(Z, Om.T, Om.P, col.Tk[k], col.Pk[k]), floor=1e-300) < 1e-11
    ctx.close()


def test_batch_accel_shards(cs, lines, h2o):
    nu = np.linspace(1500.0, 1700.0, 6000)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    gases = [cs.DirectGas(h2o, W.fC_h2o, nu, shape="voigtCKD"), cs.DirectGas(lines("CO2"), 400e-6, nu)]
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
    # cs_accel_store over a code-4 column = sigma_fetch of that column at the knots
    Pe = cs.pressuregrid(10.0, 1e5, 12)
    Te = np.clip(W.earth_temperature(Pe), 160.0, 340.0)
    A = cs.AcceleratedAbsorber(Te, Pe, *gases, ctx=ctx)
    kcol = A._knots
    kcol.sigma_run()
    s = kcol.sigma_nodes()
    kn = np.zeros((len(Pe), len(nu)))
    cs.check(cs.lib().cs_accel_fetch(ctx.handle, A.slot, len(nu), len(Pe), cs.dptr(kn)))
    tiny = np.finfo(float).tiny
    with np.errstate(divide="ignore"):
        ls = np.maximum(np.log(s), np.log(tiny))
    assert not np.any(np.isnan(kn)) and np.max(np.abs(kn - ls)) < 1e-14 * np.max(np.abs(ls))
    # two nu-ranges, and MultiContext with two contexts, add up to the whole
    F = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=ctx)
    parts = [cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=ctx, nu_range=r) for r in ((0, 2500), (2500, 6000))]
    Fu = 0.0
    for c in parts:
        c.run()
        Fu = Fu + c.fetch()[0]
    assert np.max(np.abs(Fu - F.Fup)) < 1e-12 * np.max(F.Fup)
    mc = cs.MultiContext([0, 0])
    G = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=mc)
    assert np.max(np.abs(G.Fup - F.Fup)) < 1e-12 * np.max(F.Fup) and np.max(np.abs(G.tau - F.tau) / F.tau) < 1e-12
    mc.close()
    ctx.close()
