"""CS_SHAPE_PSHIFT (include/clearsky_hip.h): HITRAN's air pressure shift of the line centres on the device, through every entry point
that takes a shape.

Line l's term is the unflagged term evaluated on the grid nu - s_l, s_l = delta_l P / P0: S, alpha and gamma stay those of the
unshifted nul, so for the lines sharing one shift s the flagged sum is the oracle's shape!(base, nu - s, those lines, ...), and the
expected value is the sum of those over the distinct shifts (`expected`).  The library takes the shifts from the .par file (the native
parser), so tables with chosen shifts are written as .par files first (`write_par`).  With delta a multiple of 2^-5 (what the
8-character field holds exactly) and P a dyadic multiple of P0, nul + s and nu - s are exact in fp64 and the device agrees with the
oracle to the suite's 1e-11.  With arbitrary delta and P the
device rounds nul + s once and the oracle rounds nu - s once: the distance moves by about 1 ulp(nu), 1e-13 cm^-1 near 1000 cm^-1;
near a core of Doppler width alpha ~ 1.6e-3 cm^-1 the profile's relative slope is ~ 1/alpha, so the value moves by ~1e-10 of it --
those comparisons use 1e-9.
"""
import os

import numpy as np
import pytest

import workloads as W
from conftest import HITRAN, relerr
from par_files import write_par

pytestmark = pytest.mark.gpu

CUT = 25.0
KATM = 101325.0
PSHIFT = 16
EINVAL = -1
BASES = ["voigt", "lorentz", "doppler"]


class _Tab:
    pass


def subset(sl, m):
    o = _Tab()
    for n in ("nu", "S", "gamma_a", "gamma_s", "Epp", "na", "mu", "I"):
        setattr(o, n, np.ascontiguousarray(getattr(sl, n)[m]))
    o.ncheb, o.cheb = sl.ncheb, sl.cheb
    return o


def expected(O, sl, da, base, nu, T, P, Pp, strict, cut=CUT):
    """sum over the distinct shifts s of the oracle's shape! of the lines with that shift on the grid nu - s"""
    nu = np.asarray(nu, float)
    s_l = np.asarray(da, float) * P / KATM
    near = (sl.nu > nu[0] - cut - 2.0) & (sl.nu < nu[-1] + cut + 2.0)   # (shifts here stay below 1 cm^-1: the others add nothing)
    out = np.zeros(len(nu))
    for s in np.unique(s_l[near]):
        out += O.shape_bang(base, nu - s, subset(sl, near & (s_l == s)), T, P, Pp, cut, strict_ends=strict)
    return out


def with_delta(cs, tmp, name, sl, da):
    """sl's lines with the shifts da, through a .par file"""
    return cs.SpectralLines(write_par(os.path.join(tmp, name + ".par"), sl.M, sl.nu, sl.S, sl.gamma_a, sl.gamma_s, sl.Epp, sl.na, da, sl.I))


def synthetic(cs, tmp, name, da_choice, seed=7, L=50000, numax=2525.0, M=1):
    """a dense seeded table (a line every 0.05 cm^-1) with shifts drawn from da_choice"""
    rng = np.random.default_rng(seed)
    nu = np.unique(np.round(rng.uniform(0.0, numax, L), 6))
    n = len(nu)
    da = rng.choice(da_choice, n)
    return cs.SpectralLines(write_par(os.path.join(tmp, name + ".par"), M, nu, 10.0 ** rng.uniform(-28, -19, n), rng.uniform(0.05, 0.10, n),
                                      rng.uniform(0.06, 0.13, n), rng.uniform(0, 3000, n), rng.uniform(0.6, 0.8, n), da))


def dyadic(da):
    return np.round(np.asarray(da) * 32.0) / 32.0


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("pshift"))


def exact_premise(nul, nu, da, Ps):
    """nul + s and nu - s are exact in fp64 (compared with extended precision where the platform has it)"""
    L = np.longdouble
    for P in Ps:
        s = da * P / KATM
        assert np.all(s == da * (P / KATM))
        assert np.all(L(nul) + L(s) == L(nul + s))
        for sv in np.unique(s):
            assert np.all(L(nu) - L(sv) == L(nu - sv))


@pytest.fixture(scope="module")
def ctx(cs):
    c = cs.Context(0)
    yield c
    c.close()


GRIDS = {"H2O": (1300.0, 1700.0), "CO2": (600.0, 760.0)}


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("gas", ["H2O", "CO2"])
def test_exact_shifts_b1(cs, O, ctx, lines, tmp, gas, base):
    sl0 = lines(gas)
    sl = with_delta(cs, tmp, gas + "_dyadic", sl0, dyadic(sl0.delta_a))
    da = sl.delta_a
    assert np.array_equal(da, dyadic(sl0.delta_a)) and np.any(da != 0)
    nu = np.linspace(*GRIDS[gas], 4001)
    P = [0.25 * KATM, KATM, 2.0 * KATM]
    T, Pp = [250.0, 296.0, 310.0], [100.0, 2000.0, 500.0]
    near = (sl.nu > nu[0] - CUT - 2.0) & (sl.nu < nu[-1] + CUT + 2.0)
    exact_premise(sl.nu[near], nu, da[near], P)
    sv = cs.shape_batch(sl, base, nu, T, P, Pp, CUT, ctx, pressure_shift=True)
    sp = cs.shape_points(sl, base, nu, T, P, Pp, CUT, ctx, pressure_shift=True)
    s0 = cs.shape_batch(sl, base, nu, T, P, Pp, CUT, ctx)
    for k in range(3):
        for s, strict in ((sv[k], True), (sp[k], False)):
            r = expected(O, sl, da, base, nu, T[k], P[k], Pp[k], strict)
            assert np.max(np.abs(s - r)) < 1e-11 * np.max(np.abs(r)), (k, strict)
        # the shift moves the peaks by about a line width at 1 atm: far more than rounding (the Doppler cores, 1e-3 cm^-1 wide, fall
        # between the points of this grid)
        if k > 0 and base != "doppler" and gas == "H2O":   # (CO2's shifts, below 0.02 cm^-1/atm, round to 0 or 2^-5)
            assert np.max(np.abs(sv[k] - s0[k])) > 1e-3 * np.max(s0[k])
    # the in-place and scalar forms
    if base == "voigt":
        s = np.zeros_like(nu)
        assert cs.voigt_(s, nu, sl, T[1], P[1], Pp[1], ctx=ctx, pressure_shift=True) is None
        # (not bit for bit: a one-state call widens its windows and zones by that state's shift, the batch by the largest of three, so
        # a few lines take another series body -- each exact to 1e-15)
        assert np.max(np.abs(s - sv[1])) <= 1e-14 * np.max(sv[1])
        assert cs.voigt(float(nu[1234]), sl, T[1], P[1], Pp[1], ctx=ctx, pressure_shift=True) == pytest.approx(sp[1][1234], rel=1e-13)


def test_realistic_shifts_b1(cs, O, ctx, lines):
    """the file's own delta_a at arbitrary pressures (1e-9: see the module docstring)"""
    sl = lines("H2O")
    assert np.mean(sl.delta_a != 0) > 0.8
    nu = np.linspace(1350.0, 1650.0, 3001)
    T, P, Pp = [230.0, 290.0], [87654.3, 3123.4], [1234.5, 10.0]
    for base in BASES:
        sv = cs.shape_batch(sl, base, nu, T, P, Pp, CUT, ctx, pressure_shift=True)
        sp = cs.shape_points(sl, base, nu, T, P, Pp, CUT, ctx, pressure_shift=True)
        for k in range(2):
            for s, strict in ((sv[k], True), (sp[k], False)):
                r = expected(O, sl, sl.delta_a, base, nu, T[k], P[k], Pp[k], strict)
                assert np.max(np.abs(s - r)) < 1e-9 * np.max(np.abs(r)), (base, k, strict)


def _column(cs, ctx, gases, P, T, **kw):
    return cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=ctx, **kw)


NU0, DNU = 0.5, 0.008


def test_zero_shift_equals_unflagged(cs, tmp):
    """delta = 0: the flagged column equals the unflagged one, which runs the matrix-core forms; the flagged one keeps the interpolated
    far wings on the vector node sums and runs no matrix-core kernel"""
    sz = synthetic(cs, tmp, "zero", [0.0])
    assert np.all(sz.delta_a == 0)
    nu = NU0 + DNU * np.arange(64 * 2000)
    P = cs.pressuregrid(10.0, 1e5, 61)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    res = {}
    for flag in (False, True):
        col = _column(cs, ctx, [cs.DirectGas(sz, W.fC_h2o, nu, pressure_shift=flag)], P, T)
        col.run()
        res[flag] = (col.sigma_nodes(), col.work(), col.info())
    (a, wa, ia), (b, wb, ib) = res[False], res[True]
    assert wa["edge_mx_flops_useful"] > 0 and wa["node_evals"] > 0, wa
    assert wb["node_evals"] > 0 and wb["levels"] > 0, wb
    assert wb["edge_mx_flops_useful"] == 0 and wb["node_evals_matrix"] == 0 and wb["nodes_mx_flops_useful"] == 0, wb
    assert ib["line_kernel"] == 0, ib   # (k_voigt_far)
    assert np.max(np.abs(a - b)) < 5e-13 * np.max(a)
    ctx.close()


@pytest.mark.parametrize("base", BASES)
def test_edges_one_line(cs, O, ctx, lines, tmp, base):
    """one line whose shift carries grid points across the inclusive +-cut boundary and across the strict grid-end pre-filter"""
    sl0 = lines("CO2")
    l = int(np.argmin(np.abs(sl0.nu - 700.0)))
    d = -0.25                                   # delta [cm^-1/atm]; at 2 atm the centre moves by -0.5

    def one_line(name, dv):
        return cs.SpectralLines(write_par(os.path.join(tmp, name + ".par"), 2, sl0.nu[l:l + 1], sl0.S[l:l + 1], sl0.gamma_a[l:l + 1],
                                          sl0.gamma_s[l:l + 1], sl0.Epp[l:l + 1], sl0.na[l:l + 1], [dv], sl0.I[l:l + 1]))
    one = one_line(f"one_down_{base}", d)
    P, T, Pp = 2.0 * KATM, 296.0, 100.0
    nl, s = one.nu[0], d * P / KATM
    c = nl + s
    eps = np.array([1e-3, 1e-6])
    nu = np.unique(np.concatenate([np.linspace(c - 40.0, c + 40.0, 801), c + CUT + eps, c + CUT - eps, [c + CUT, c - CUT],
                                   c - CUT + eps, c - CUT - eps, nl + CUT + eps, nl - CUT - eps]))
    sv = cs.shape_points(one, base, nu, [T], [P], [Pp], CUT, ctx, pressure_shift=True)[0]
    r = expected(O, one, one.delta_a, base, nu, T, P, Pp, False)
    assert np.max(np.abs(sv - r)) < 1e-11 * np.max(r)
    inside = np.abs(nu - c) <= CUT
    assert np.all(sv[~inside] == 0.0)
    if base == "doppler":   # (the Doppler profile is an exact zero in fp64 long before the cut-off: no edge to see)
        return
    assert np.all(sv[inside] > 0.0)
    assert sv[nu == c + CUT][0] > 0 and sv[nu == c - CUT][0] > 0
    # strict pre-filter from the shifted centre: a grid ending where nul + s < nu_N + cut <= nul keeps the line ...
    g1 = np.linspace(c - CUT - 5.0, c - CUT + 0.25, 101)      # nu_N + cut = c + 0.25 < nl = c + 0.5
    assert g1[-1] + CUT > c and g1[-1] + CUT < nl
    a1 = cs.shape_batch(one, base, g1, [T], [P], [Pp], CUT, ctx, pressure_shift=True)[0]
    assert np.any(a1 > 0) and np.max(np.abs(a1 - expected(O, one, one.delta_a, base, g1, T, P, Pp, True))) < 1e-11 * np.max(a1)
    # ... and one ending where nul < nu_N + cut <= nul + s of a line shifted upwards drops it
    up = one_line(f"one_up_{base}", -d)
    g2 = np.linspace(nl - CUT - 5.0, nl - CUT + 0.25, 101)     # nl < nu_N + cut = nl + 0.25 < nl + 0.5
    a2 = cs.shape_batch(up, base, g2, [T], [P], [Pp], CUT, ctx, pressure_shift=True)[0]
    b2 = cs.shape_batch(up, base, g2, [T], [P], [Pp], CUT, ctx)[0]
    assert np.all(a2 == 0.0) and np.any(b2 > 0)


def _sample(n):
    last = n - ((n - 1) % 64 + 1)
    mid = np.random.default_rng(n).choice(np.arange(64, last), 64, replace=False)
    return np.unique(np.concatenate([np.arange(64), mid, np.arange(last, n)]))


def test_long_grid_interp_on_off(cs, O, tmp):
    """a dense table (a line every 0.05 cm^-1), delta from four dyadic values, shifts of up to 0.5 cm^-1 -- across interval and tile
    classifications of the table positions: interpolation on and off agree and match the oracle (1e-9: a few lines near a power of two
    round nul + s, the module docstring's case); a column over it runs the vector node sums, the far and near-line kernels, and no
    matrix-core kernel"""
    sl = synthetic(cs, tmp, "dense4", [-0.5, -0.25, 0.25, 0.5])
    da = sl.delta_a
    assert set(np.unique(da)) == {-0.5, -0.25, 0.25, 0.5}
    n = 100000
    nu = NU0 + DNU * np.arange(n)
    T = list(np.linspace(200.0, 310.0, 8))
    P = [KATM * f for f in (0.125, 0.25, 0.5, 1.0, 1.0, 0.5, 0.25, 1.0)]
    Pp = [0.01 * p for p in P]
    idx = _sample(n)
    x = nu[idx]
    assert x[0] == nu[0] and x[-1] == nu[-1]   # (the strict pre-filter of the whole grid)
    for base in ("voigt", "lorentz"):
        res = {}
        for on in (True, False):
            c = cs.Context(0)
            c.set_interp(on)
            res[on] = cs.shape_batch(sl, base, nu, T, P, Pp, CUT, c, pressure_shift=True)
            c.close()
        assert relerr(res[True], res[False], floor=1e-280) < 2e-13, base
        for k in range(0, 8, 3):
            r = expected(O, sl, da, base, x, T[k], P[k], Pp[k], True)
            for on in (True, False):
                assert np.max(np.abs(res[on][k][idx] - r)) < 1e-9 * np.max(r), (base, k, on)
    ctx = cs.Context(0)
    Pc = cs.pressuregrid(10.0, 1e5, 9)
    col = _column(cs, ctx, [cs.DirectGas(sl, W.fC_h2o, nu[:64 * 600], pressure_shift=True)], Pc, W.earth_temperature(Pc))
    col.run()
    w, i = col.work(), col.info()
    assert i["line_kernel"] == 0 and w["levels"] > 0 and w["node_evals"] > 0, (i, w)                    # k_voigt_far, k_cheb_nodes
    assert w["near_pairs_tier0"] + w["near_pairs_tier1"] > 0, w                                          # k_voigt_near
    assert w["node_evals_matrix"] == 0 and w["nodes_mx_flops_useful"] == 0 and w["edge_mx_flops_useful"] == 0, w
    # the sums of that column against the oracle at sampled points of its grid
    sig = col.sigma_nodes()
    xs = nu[:64 * 600][_sample(64 * 600)]
    j = np.searchsorted(nu, xs)
    ex = node_expected(O, col, 0, xs, da)
    assert np.max(np.abs(sig[:, j] - ex)) < 1e-9 * np.max(ex)
    ctx.close()


def node_expected(O, col, gi, x, da, base="voigt"):
    g = col.gases[gi]
    out = np.zeros((col.K, len(x)))
    for k in range(col.K):
        Ck = col.conc[gi, k]
        out[k] = Ck * expected(O, g.sl, da, base, x, col.Tk[k], col.Pk[k], Ck * col.Pk[k], False)
    return out


def _fetch(col):
    col.run()
    tau = np.zeros((col.nl, col.nnu), order="F")
    Mu = np.zeros((col.np, col.nnu), order="F")
    Md = np.zeros((col.np, col.nnu), order="F")
    Fup, Fdn = col.fetch(tau, Mu, Md)
    return dict(tau=tau, Mup=Mu, Mdn=Md, Fup=Fup, Fdn=Fdn)


FORMS = [(300, {15: 1}), (600, {}), (4200, {})]


@pytest.mark.parametrize("tiles,tune", FORMS, ids=[f"{t}tiles{'-unfused' if u else ''}" for t, u in FORMS])
def test_column(cs, O, lines, tiles, tune):
    """flagged H2O beside unflagged CO2 in one column: sigma at the nodes against the oracle sum, fluxes against the oracle column of
    CO2 with C x sigma of H2O as sigma_extra"""
    n = 64 * tiles
    nu = np.linspace(1200.0, 1800.0, n) if tiles < 4000 else np.linspace(500.0, 2500.0, n)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    for k_, v in tune.items():
        ctx.set_tuning(k_, v)
    h2o = lines("H2O")
    gases = [cs.DirectGas(h2o, W.fC_h2o, nu, pressure_shift=True), cs.DirectGas(lines("CO2"), 400e-6, nu)]
    col = _column(cs, ctx, gases, P, T)
    r = _fetch(col)
    idx = np.arange(n) if n <= 20000 else _sample(n)
    ex = node_expected(O, col, 0, nu[idx], h2o.delta_a)
    ref = O.fluxes_discretized(nu[idx], col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [lines("CO2")], ["voigt"], [CUT], col.conc[1:],
                               sigma_extra=ex, theta_s=col.theta_s, nstream=col.core.nstream, want_sigma=True)
    sig = col.sigma_nodes()[:, idx]
    assert np.max(np.abs(sig - ref["sigma"])) < 1e-9 * np.max(ref["sigma"])
    assert relerr(r["tau"][:, idx], ref["tau"]) < 1e-9
    sm = max(ref["Mup"].max(), ref["Mdn"].max())
    for k in ("Mup", "Mdn"):
        assert np.max(np.abs(r[k][:, idx] - ref[k])) < 1e-9 * sm, k
    if n <= 20000:
        for k in ("Fup", "Fdn"):
            assert np.max(np.abs(r[k] - ref[k])) < 1e-9 * np.max(ref["Fup"]), k
    ctx.close()


def test_merge_and_bake(cs, lines):
    """two flagged Voigt gases merge into one group and equal the separate groups; a flagged gas does not merge with an unflagged one;
    cs_bake's knots are ln of B1 at the knot states"""
    nu = np.linspace(1000.0, 1600.0, 6000)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    co2 = lines("CO2")
    a = cs.DirectGas(lines("H2O"), W.fC_h2o, nu, pressure_shift=True)
    b = cs.DirectGas(co2, 400e-6, nu, pressure_shift=True)
    u = cs.DirectGas(lines("CO2"), 400e-6, nu)
    out = {}
    for merge in (True, False):
        ctx.set_merge(merge)
        col = _column(cs, ctx, [a, b, u], P, T)
        col.sigma_run()
        out[merge] = (col.sigma_nodes(), col.info()["groups"])
    ctx.set_merge(True)
    assert out[True][1] == 2 and out[False][1] == 3
    assert np.max(np.abs(out[True][0] - out[False][0])) < 5e-13 * np.max(out[False][0])
    Om = cs.AtmosphericDomain((150.0, 350.0), 12, (10.0, 1e5), 24)
    g = cs.Gas(lines("H2O"), 0.01, nu, Om, ctx=ctx, keep_host_tables=True, pressure_shift=True)
    TT, PP = np.meshgrid(Om.T, Om.P, indexing="ij")
    s = cs.shape_batch(lines("H2O"), "voigt", nu, TT.ravel(order="F"), PP.ravel(order="F"), 0.01 * PP.ravel(order="F"), CUT, ctx,
                       pressure_shift=True)
    ref = np.log(np.maximum(s.T.reshape(len(nu), Om.nT, Om.nP, order="F"), np.finfo(float).tiny))
    assert np.max(np.abs(g.lnsigma - ref)) < 1e-12 * np.max(np.abs(ref))
    ctx.close()


def test_batch_accel_shards(cs, lines, tmp):
    """cs_column_batch against sequential runs, cs_accel_store against the column's sigma, and nu-shards adding up to the whole, where
    lines just outside a shard's unshifted reach shift into it"""
    n = 6000
    nu = np.linspace(1000.0, 1120.0, n)
    P = cs.pressuregrid(10.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    # lines at the edges of the reach of the two shards' grids, shifted inwards by 0.5 cm^-1 at the surface
    sl0 = lines("H2O")
    edge = nu[2500]
    extra = np.array([nu[0] - CUT - 0.3, edge - CUT - 0.3, nu[2499] + CUT + 0.3, nu[-1] + CUT + 0.3])
    sh = [0.5, 0.5, -0.5, -0.5]
    m = (sl0.nu > 900.0) & (sl0.nu < 1220.0)
    par = {k: np.asarray(getattr(sl0, k))[m] for k in ("nu", "S", "gamma_a", "gamma_s", "Epp", "na", "delta_a")}
    j = int(np.argmax(par["S"]))
    for x, d in zip(extra, sh):
        for k in par:
            par[k] = np.append(par[k], par[k][j] if k != "nu" else x)
        par["delta_a"][-1] = d
    o = np.argsort(par["nu"], kind="stable")
    p = {k: v[o] for k, v in par.items()}
    sl = cs.SpectralLines(write_par(os.path.join(tmp, "shards.par"), 1, p["nu"], p["S"], p["gamma_a"], p["gamma_s"], p["Epp"], p["na"],
                                    p["delta_a"]))
    assert np.sum(np.abs(sl.delta_a) == 0.5) == 4
    gases = [cs.DirectGas(sl, W.fC_h2o, nu, pressure_shift=True), cs.DirectGas(lines("CO2"), 400e-6, nu)]
    col = _column(cs, ctx, gases, P, T, want_tau=False, want_M=False)
    Tlev = np.array(col.Tlev)
    Ts = [Tlev] + [Tlev + 1.0 * (np.arange(len(P)) == i) for i in range(0, len(P), 3)]
    Bu, Bd = col.run_batch(Ts, 0.029)
    for b, Tb in enumerate(Ts):
        one = _column(cs, ctx, gases, P, cs.AtmosphericProfile(P, Tb), want_tau=False, want_M=False)
        one.run()
        Fu, Fd = one.fetch()
        assert np.max(np.abs(Bu[b] - Fu)) < 5e-13 * np.max(Fu) and np.max(np.abs(Bd[b] - Fd)) < 5e-13 * np.max(Fu)
    Pe = cs.pressuregrid(10.0, 1e5, 12)
    Te = np.clip(W.earth_temperature(Pe), 160.0, 340.0)
    A = cs.AcceleratedAbsorber(Te, Pe, *gases, ctx=ctx)
    kcol = A._knots
    kcol.sigma_run()
    s = kcol.sigma_nodes()
    kn = np.zeros((len(Pe), len(nu)))
    cs.check(cs.lib().cs_accel_fetch(ctx.handle, A.slot, len(nu), len(Pe), cs.dptr(kn)))
    assert np.max(np.abs(kn - np.log(s))) < 1e-14 * np.max(np.abs(np.log(s)))
    # the same knots through B1 (scalar-nu method: the column's)
    for k in (0, len(Pe) - 1):
        C_ = W.fC_h2o(kcol.Tk[k], kcol.Pk[k])
        b1 = C_ * cs.shape_points(sl, "voigt", nu, [kcol.Tk[k]], [kcol.Pk[k]], [C_ * kcol.Pk[k]], CUT, ctx, pressure_shift=True)[0] + \
            400e-6 * cs.shape_points(lines("CO2"), "voigt", nu, [kcol.Tk[k]], [kcol.Pk[k]], [400e-6 * kcol.Pk[k]], CUT, ctx)[0]
        assert np.max(np.abs(s[k] - b1)) < 1e-12 * np.max(b1)
    F = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=ctx)
    Fu = 0.0
    for r in ((0, 2500), (2500, n)):
        c = cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=ctx, nu_range=r)
        c.run()
        Fu = Fu + c.fetch()[0]
    assert np.max(np.abs(Fu - F.Fup)) < 1e-12 * np.max(F.Fup)
    mc = cs.MultiContext([0, 0])
    G = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=mc)
    assert np.max(np.abs(G.Fup - F.Fup)) < 1e-12 * np.max(F.Fup)
    mc.close()
    ctx.close()


def test_refusals(cs, lines):
    ctx = cs.Context(0)
    L = cs.lib()
    sl = lines("CO2")
    slot = ctx.slot_of(sl, shift=True)
    nu = np.linspace(600.0, 700.0, 101)
    T, P, Pp = np.array([296.0]), np.array([KATM]), np.array([40.0])
    out = np.zeros(len(nu))

    def call(code, slot_=slot):
        return L.cs_shape_batch(ctx.handle, slot_, code, CUT, len(nu), cs.dptr(nu), 1, cs.dptr(T), cs.dptr(P), cs.dptr(Pp), cs.dptr(out),
                                len(nu))
    for base in (0, 1, 2):
        assert call(base | PSHIFT) == 0
    for code in (3, 4, 5, 6):
        assert call(code | PSHIFT) == EINVAL
    for code in (32, 0 | 64, PSHIFT | 32, 7 | PSHIFT):
        assert call(code) == EINVAL
    # a slot filled from arrays (cs_gas_upload) has no shifts and refuses the flag -- never a shift of zero
    par = {k: getattr(sl, k) for k in ("nu", "S", "gamma_a", "gamma_s", "Epp", "na")}
    bare = cs.SpectralLines(dict(M=np.full(len(sl.nu), 2, np.int16), I=sl.I, A=np.zeros(len(sl.nu)), **par))
    assert bare.source is None
    s2 = ctx.slot_of(bare)
    assert call(PSHIFT, s2) == EINVAL and call(0, s2) == 0
    with pytest.raises(ValueError):   # (refused in Python first, with the reason)
        cs.shape_batch(bare, "voigt", nu, T, P, Pp, CUT, ctx, pressure_shift=True)
    # a file-backed table whose arrays were changed after reading cannot take the file's shifts: refused, and its own table stays
    mod = cs.SpectralLines(os.path.join(HITRAN, "CO2.par"))
    mod.S = mod.S * 2.0
    plain = cs.shape_batch(mod, "voigt", nu, T, P, Pp, CUT, ctx)
    with pytest.raises(ValueError):
        cs.shape_batch(mod, "voigt", nu, T, P, Pp, CUT, ctx, pressure_shift=True)
    assert np.array_equal(cs.shape_batch(mod, "voigt", nu, T, P, Pp, CUT, ctx), plain)
    # a re-upload through cs_gas_upload drops the shifts a .par load gave the slot
    assert call(PSHIFT) == 0
    arrs = [cs.as_f64(a) for a in (sl.nu, sl.S, sl.gamma_a, sl.gamma_s, sl.Epp, sl.na, sl.mu)]
    iso = np.ascontiguousarray(sl.I, dtype=np.int16)
    ncheb = np.ascontiguousarray(sl.ncheb, dtype=np.int32)
    cheb = cs.as_f64(sl.cheb)
    import ctypes as C
    assert L.cs_gas_upload(ctx.handle, slot, len(arrs[0]), *[cs.dptr(a) for a in arrs], iso.ctypes.data_as(C.POINTER(C.c_int16)),
                           len(ncheb), ncheb.ctypes.data_as(C.POINTER(C.c_int32)), cs.dptr(cheb)) == 0
    assert call(PSHIFT) == EINVAL and call(0) == 0
    # the native parser attaches the file's own shifts
    sp = ctx.load_par(os.path.join(HITRAN, "CO2.par"), 2)
    a = cs.shape_batch(sp, "voigt", nu, T, P, Pp, CUT, ctx, pressure_shift=True)
    ctx2 = cs.Context(0)
    b = cs.shape_batch(sl, "voigt", nu, T, P, Pp, CUT, ctx2, pressure_shift=True)
    ctx2.close()
    assert np.max(np.abs(a - b)) <= 1e-14 * np.max(b)
    ctx.close()
