"""Shape code 5, the Van Vleck-Huber Voigt (include/clearsky_hip.h, CS_SHAPE_VOIGT_VVH), on the device through every entry point that
takes a shape.

The oracle knows only the reference's four shapes, so the expected values are assembled from its Voigt:
  sigma_5(nu) = R(nu, T) [voigt~(nu) + sum_{l: nu + nul <= cut} voigt~_l(2 nul + nu)],   R(x, T) = x tanh(c2 x / 2T)
voigt~ is the oracle's Voigt of the table with every S_l scaled by S~_l / S_l = (1 + e^(-c2 nul/T)) / (nul (1 - e^(-c2 nul/T))), the
factor 1 / R(nul, T) with the oracle's own rounding of 1 - e^(-c2 nul/T) taken out (math.exp is the oracle's exp); voigt~_l is that
of the ONE-line slice l, evaluated at 2 nul + nu, which has dnu = nu + nul and the same alpha and gamma (the mirror term).  The
restatement itself is checked against 40-digit arithmetic in test_voigt_vvh.py.  Columns compare against the oracle column of the
other gases with sigma_extra = C x sigma_5 at every node.  Tolerances are the suite's: 1e-11 against the oracle, 5e-13 device
against device, 2e-13 interpolation on against off.
"""
import math
import os

import numpy as np
import pytest

import workloads as W
from clearsky_jl_amd import DISPATCH_FLAGS
from conftest import HITRAN, relerr

pytestmark = pytest.mark.gpu

CUT = 25.0
STATES = [(220.0, 50.0, 0.02), (296.0, 101325.0, 40.53), (260.0, 3e3, 30.0)]
RT_STREAMS = DISPATCH_FLAGS["RT_STREAMS"]   # Column.work()["dispatch"]["flags"]


def c2(cs):
    C_ = cs.constants
    return 100.0 * C_.h * C_.c / C_.k


def R(cs, x, T):
    return x * np.tanh(c2(cs) * x / (2.0 * T))


class _Tab:
    pass


def tilde(cs, sl, T, a=0, b=None):
    """the lines [a, b) of sl with S scaled so that the oracle's S_l(T) becomes S_l(T) / R(nul, T)"""
    b = len(sl.nu) if b is None else b
    o = _Tab()
    for n in ("nu", "S", "gamma_a", "gamma_s", "Epp", "na", "mu", "I"):
        setattr(o, n, np.ascontiguousarray(getattr(sl, n)[a:b]))
    o.ncheb, o.cheb = sl.ncheb, sl.cheb
    k2 = c2(cs)
    f = []
    for nl in o.nu:
        e = math.exp(-k2 * nl / T)
        f.append((1.0 + e) / (nl * (1.0 - e)))
    o.S = o.S * np.array(f)
    return o


def expected(cs, O, sl, nu, T, P, Pp, cut=CUT, strict=True, t=None):
    nu = np.asarray(nu, float)
    t = tilde(cs, sl, T) if t is None else t
    s = O.shape_bang("voigt", nu, t, T, P, Pp, cut, strict_ends=strict)
    keep = (sl.nu > nu[0] - cut) & (sl.nu < nu[-1] + cut) if strict else np.ones(len(sl.nu), bool)
    for l in np.nonzero(keep & (sl.nu <= cut - nu[0] + 1e-9))[0]:
        m = ~(nu + sl.nu[l] > cut)
        if m.any():
            s[m] += O.shape_bang("voigt", 2.0 * sl.nu[l] + nu[m], tilde(cs, sl, T, l, l + 1), T, P, Pp, 2.0 * cut, strict_ends=False)
    return R(cs, nu, T) * s


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
    nu = np.unique(np.concatenate([[0.0, 1e-6, 1e-3], np.linspace(0.01, 110.0, 6001)]))
    T, P, Pp = map(list, zip(*STATES))
    sv = cs.shape_batch(h2o_low, "voigtVVH", nu, T, P, Pp, CUT, ctx)
    sp = cs.shape_points(h2o_low, "voigtVVH", nu, T, P, Pp, CUT, ctx)
    v0 = cs.shape_batch(h2o_low, "voigt", nu, T, P, Pp, CUT, ctx)
    for k in range(len(T)):
        rv = expected(cs, O, h2o_low, nu, T[k], P[k], Pp[k], strict=True)
        rp = expected(cs, O, h2o_low, nu, T[k], P[k], Pp[k], strict=False)
        for s, r in ((sv[k], rv), (sp[k], rp)):
            assert np.all(np.isfinite(s)) and np.all(s >= 0)
            assert s[0] == 0.0                                   # nu = 0
            assert relerr(s, r, floor=1e-300) < 1e-11, k
        # the low-wavenumber wings differ from plain Voigt by far more than rounding
        m = nu > 1.0
        assert np.max(np.abs(sv[k][m] / v0[k][m] - 1.0)) > 0.3
    s = np.zeros_like(nu)
    assert cs.voigtVVH_(s, nu, h2o_low, T[1], P[1], Pp[1], ctx=ctx) is None
    assert np.array_equal(s, sv[1])
    assert np.array_equal(cs.voigtVVH(nu, h2o_low, T[1], P[1], Pp[1], ctx=ctx), sv[1])
    # the scalar method on a one-point grid: the same lines, summed without the interpolated wings of the long grid
    assert abs(cs.voigtVVH(float(nu[777]), h2o_low, T[1], P[1], Pp[1], ctx=ctx) - sp[1][777]) < 1e-13 * sp[1][777]


def _one(cs, sl, l):
    return cs.SpectralLines(dict(M=np.full(1, 1, np.int16), I=sl.I[l:l + 1], nu=sl.nu[l:l + 1], S=sl.S[l:l + 1],
                                 gamma_a=sl.gamma_a[l:l + 1], gamma_s=sl.gamma_s[l:l + 1], Epp=sl.Epp[l:l + 1], na=sl.na[l:l + 1],
                                 A=np.zeros(1), delta_a=np.zeros(1)))


def test_cutoff_edges_one_line(cs, O, ctx, h2o_low):
    """both terms at exactly the cut-off: the direct term where |nu - nul| = cut, the mirror term where nu + nul = cut (inclusive),
    one step beyond each neither"""
    T, P, Pp = STATES[1]
    d = np.array([1e-1, 1e-3])
    for target in (10.0, 100.0):
        l = int(np.argmin(np.abs(h2o_low.nu - target)))
        one = _one(cs, h2o_low, l)
        nl = one.nu[0]
        edges = [nl + CUT, CUT - nl, nl - CUT]
        nu = np.concatenate([np.linspace(0.0, nl + 40.0, 801), *[[e, e - dd, e + dd] for e in edges for dd in d]])
        nu = np.unique(nu[nu >= 0.0])
        for s, strict in ((cs.shape_batch(one, "voigtVVH", nu, [T], [P], [Pp], CUT, ctx)[0], True),
                          (cs.shape_points(one, "voigtVVH", nu, [T], [P], [Pp], CUT, ctx)[0], False)):
            r = expected(cs, O, one, nu, T, P, Pp, strict=strict)
            assert relerr(s, r, floor=1e-300) < 1e-11, (target, strict)
            out = (np.abs(nu - nl) > CUT) & (nu + nl > CUT)
            assert np.all(s[out] == 0.0) and np.all(s[~out & (nu > 0)] > 0)
            if nl < CUT:   # the mirror term drops at nu = cut - nul: the value just inside exceeds the one just outside by it
                i = np.nonzero(nu == CUT - nl)[0]
                j = np.nonzero(nu == CUT - nl + d[1])[0]
                assert len(i) == 1 and len(j) == 1 and s[i[0]] > s[j[0]] * 1.0001


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
        res[on] = cs.shape_batch(sl, "voigtVVH", nu, T, P, Pp, CUT, c)
        c.close()
    assert np.all(res[True] >= 0) and np.all(np.isfinite(res[True]))
    assert relerr(res[True], res[False], floor=1e-280) < 2e-13
    idx = _sample(n)
    sub = nu[idx]
    for k in range(0, 20, 3):
        # the strict pre-filter of the whole grid: pass its end points, drop their values
        x = np.concatenate([[nu[0]], sub, [nu[-1]]]) if sub[0] != nu[0] or sub[-1] != nu[-1] else sub
        r = expected(cs, O, sl, x, T[k], P[k], Pp[k])
        r = r[1:-1] if len(x) != len(sub) else r
        for on in (True, False):
            assert relerr(res[on][k][idx], r, floor=1e-280) < 1e-11, (k, on)


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
    """C_k sigma_5 of column gas gi at the points x and every node state"""
    g = col.gases[gi]
    out = np.zeros((col.K, len(x)))
    for k in range(col.K):
        Ck = col.conc[gi, k]
        out[k] = Ck * expected(cs, O, g.sl, x, col.Tk[k], col.Pk[k], Ck * col.Pk[k], strict=False)
    return out


def _vs_oracle(O, col, r, ref, whole):
    assert relerr(r["tau"], ref["tau"]) < 1e-11
    sm = max(ref["Mup"].max(), ref["Mdn"].max())
    for k in ("Mup", "Mdn"):
        assert np.max(np.abs(r[k] - ref[k])) < 1e-11 * sm, k
    if whole:
        for k in ("Fup", "Fdn"):
            assert np.max(np.abs(r[k] - ref[k])) < 1e-11 * np.max(ref["Fup"]), k


def test_matrix_core_forms_interp_on_off(cs, O):
    """A code-5 column (synthetic H2O, K = 61) on a 2000-tile grid from 0.5 cm^-1: with interpolation on, the interpolated far wings,
    the matrix-core node sums and the window ends on the matrix cores run, as Column.work() reports; with it off, none of them.  Both
    against the oracle column (sigma_5 as sigma_extra) and against each other"""
    sl = W.lines("synthetic", "H2O")
    n = 64 * 2000
    nu = _syn_nu(n)
    P = cs.pressuregrid(10.0, 1e5, 61)
    T = W.earth_temperature(P)
    res = {}
    for on in (True, False):
        ctx = cs.Context(0)
        ctx.set_interp(on)
        col = _column(cs, ctx, [cs.DirectGas(sl, W.fC_h2o, nu, shape="voigtVVH")], P, T)
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
    assert np.all(a["sigma"] >= 0) and np.all(np.isfinite(a["sigma"]))
    assert relerr(a["sigma"], b["sigma"], floor=1e-280) < 2e-13 and relerr(a["tau"], b["tau"]) < 2e-13
    col = a["col"]
    idx = _sample(n)
    extra = node_extra(cs, O, col, 0, nu[idx])
    ref = O.fluxes_discretized(nu[idx], col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [], [], [], np.zeros((0, col.K)), sigma_extra=extra,
                               theta_s=col.theta_s, nstream=col.core.nstream, want_sigma=True)
    for r in (a, b):
        assert relerr(r["sigma"][:, idx], ref["sigma"], floor=1e-280) < 1e-11
        _vs_oracle(O, col, {k: r[k][:, idx] for k in ("tau", "Mup", "Mdn")}, ref, False)


# every flux form the step dispatches, picked by grid size (test_gpu_dispatch): tiles, cs_set_tuning, expected (flux_form, k_rt_streams)
FORMS = [(300, {15: 1}, 0, True), (600, {}, 3, False), (600, {15: 1}, 0, False), (2000, {}, 0, False), (4200, {}, 2, False),
         (4200, {15: 1}, 0, False)]


@pytest.mark.parametrize("tiles,tune,form,streams", FORMS, ids=[f"{t}tiles-{f}{'-streams' if s else ''}{'-unfused' if u else ''}"
                                                               for t, u, f, s in FORMS])
def test_column_flux_forms(cs, O, lines, h2o_low, tiles, tune, form, streams):
    """H2O as code 5 beside CO2 as code 0 on 0.5 .. 120 cm^-1 (mirror terms in the first 25): the oracle column of CO2 with
    C x sigma_5 of H2O as sigma_extra"""
    n = 64 * tiles
    nu = np.linspace(0.5, 120.0, n)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    for k_, v in tune.items():
        ctx.set_tuning(k_, v)
    gases = [cs.DirectGas(h2o_low, W.fC_h2o, nu, shape="voigtVVH"), cs.DirectGas(lines("CO2"), 400e-6, nu)]
    col = _column(cs, ctx, gases, P, T)
    r = _fetch(col)
    assert col.info()["flux_form"] == form, col.info()
    assert bool(col.work()["dispatch"]["flags"] & RT_STREAMS) == streams, col.work()["dispatch"]
    whole = n <= 20000
    idx = np.arange(n) if whole else _sample(n)
    ref = O.fluxes_discretized(nu[idx], col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [col.gases[1].sl], ["voigt"], [CUT], col.conc[1:],
                               sigma_extra=node_extra(cs, O, col, 0, nu[idx]), theta_s=col.theta_s, nstream=col.core.nstream)
    _vs_oracle(O, col, {k: (r[k][:, idx] if k in ("tau", "Mup", "Mdn") else r[k]) for k in r}, ref, whole)
    ctx.close()


def test_merge_groups_and_repeat(cs, lines, h2o_low):
    """code 5 merges only with code 5 of the same cut-off: a code-0 gas beside it, two code-5 gases of one cut (one group) and of two
    cuts (two code-5 groups) each equal the sum of the one-gas columns; every result is bitwise the same run to run, and a graph replay
    of the step equals the eager run"""
    nu = np.linspace(0.5, 300.0, 8000)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    a = cs.DirectGas(h2o_low, W.fC_h2o, nu, shape="voigtVVH")
    cases = [(cs.DirectGas(lines("CO2"), 400e-6, nu), 2), (cs.DirectGas(lines("CO2"), 400e-6, nu, shape="voigtVVH"), 1),
             (cs.DirectGas(lines("CO2"), 400e-6, nu, shape="voigtVVH", dnu_cut=20.0), 2)]

    def sig(gs):
        c = _column(cs, ctx, gs, P, T)
        c.sigma_run()
        return c.sigma_nodes(), c
    s_a, _ = sig([a])
    assert np.all(s_a >= 0)
    for b, ngroups in cases:
        s_ab, c = sig([b, a])   # (the code-5 groups run first whatever the order of the gases)
        assert c.info()["groups"] == ngroups
        s_b, _ = sig([b])
        assert relerr(s_ab, s_a + s_b, floor=1e-300) < 5e-13
        c.sigma_run()
        assert np.array_equal(c.sigma_nodes(), s_ab)
    ctx.close()
    gctx = cs.Context(0)
    gctx.set_tuning(4, 1)
    col = _column(cs, gctx, [a, cases[2][0], cases[0][0]], P, T)   # two code-5 groups and a code-0 one
    outs = []
    for _ in range(4):        # eager, capture, replay, replay
        outs.append(_fetch(col))
    for o in outs[1:]:
        for k in ("tau", "Mup", "Mdn", "Fup", "Fdn"):
            assert np.array_equal(o[k], outs[0][k]), k
    gctx.close()


def test_bake(cs, O, h2o_low):
    """Mode T: the knots are ln of shape_batch code 5 at the knot states, and a column over the baked gas follows them"""
    ctx = cs.Context(0)
    nu = np.linspace(0.5, 100.0, 3000)
    Om = cs.AtmosphericDomain((150.0, 350.0), 12, (10.0, 1e5), 24)
    g = cs.Gas(h2o_low, 0.01, nu, Om, shape="voigtVVH", ctx=ctx, keep_host_tables=True)
    Z = g.lnsigma
    assert not np.any(np.isnan(Z))
    TT, PP = np.meshgrid(Om.T, Om.P, indexing="ij")
    s = cs.shape_batch(h2o_low, "voigtVVH", nu, TT.ravel(order="F"), PP.ravel(order="F"), 0.01 * PP.ravel(order="F"), CUT, ctx)
    ref = np.log(s.T.reshape(len(nu), Om.nT, Om.nP, order="F"))
    assert np.max(np.abs(Z - ref)) < 1e-12 * np.max(np.abs(ref))
    P = cs.pressuregrid(20.0, 9e4, 7)
    T = np.clip(W.earth_temperature(P), 160.0, 340.0)
    col = _column(cs, ctx, [g], P, T)
    col.sigma_run()
    sig = col.sigma_nodes()
    for k in range(col.K):
        assert relerr(sig[k], 0.01 * O.table_sigma(Z, Om.T, Om.P, col.Tk[k], col.Pk[k]), floor=1e-300) < 1e-11
    ctx.close()


def test_batch_accel_shards(cs, lines, h2o_low):
    nu = np.linspace(0.5, 120.0, 6000)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    gases = [cs.DirectGas(h2o_low, W.fC_h2o, nu, shape="voigtVVH"), cs.DirectGas(lines("CO2"), 400e-6, nu)]
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
    # cs_accel_store over a code-5 column = sigma_fetch of that column at the knots
    Pe = cs.pressuregrid(10.0, 1e5, 12)
    Te = np.clip(W.earth_temperature(Pe), 160.0, 340.0)
    A = cs.AcceleratedAbsorber(Te, Pe, *gases, ctx=ctx)
    kcol = A._knots
    kcol.sigma_run()
    s = kcol.sigma_nodes()
    kn = np.zeros((len(Pe), len(nu)))
    cs.check(cs.lib().cs_accel_fetch(ctx.handle, A.slot, len(nu), len(Pe), cs.dptr(kn)))
    assert not np.any(np.isnan(kn)) and np.max(np.abs(kn - np.log(s))) < 1e-14 * np.max(np.abs(np.log(s)))
    # two nu-ranges (the first holds the mirror terms), and MultiContext with two contexts, add up to the whole
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
