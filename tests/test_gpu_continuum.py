"""CIA objects flagged CS_CIA_RADIATION (include/clearsky_hip.h) and the Continuum built on them, on the device: columns whose
cross-section is the flagged term alone, through the plane form (k_cia<true>), the three flux forms (k_cia_tab + cia_add<true> in k_flux_scan
/ k_flux_chunk*, and the separate kernels), update, batches, the accelerated absorber and fluxes().  Mirrors tests/test_gpu_cia_bands.py,
whose helpers it uses.

Reference: tabulated_ref.cia_sigma x R(nu, T) with R = nu tanh(c2 nu / 2T) in mpmath at 40 digits (tests/continuum_ref.py); optical
depths and fluxes from the oracle fed that plane as sigma_extra.  Tolerances: sigma and tau 4 x (tabulated_ref.cia_bound + 8 x 2^-53)
-- the three roundings of the argument, the tanh and two products, with the condition number of x tanh x at most 2 -- and the flux rule
of tests/test_gpu_cia_bands.py unchanged.  Two grids (continuum_ref.grid): above the CO2 fixture's last line, and 0.5 .. 80 cm^-1, where
tanh is in its small-argument regime.  Every case prints its largest error / bound ratio (pytest -s).
"""
import ctypes as C

import numpy as np
import pytest

import continuum_ref as CR
import tabulated_ref as R
import test_gpu_cia_bands as B

pytestmark = pytest.mark.gpu

FORMS = B.FORMS
SYMBOL = {"high": "CO2-CO2", "low": "H2O-H2O"}
X1 = 0.9                                           # concentration of the one line gas: both partial pressures are 0.9 P


def _gas(cs, lines, which, nu):
    sl = lines("CO2") if which == "high" else CR.low_lines(cs)
    assert (sl.nu.max() + 25.0 < nu[0]) if which == "high" else (sl.nu.min() - 25.0 > nu[-1])
    return cs.DirectGas(sl, X1, nu)


def _pgrid(cs, np_):
    return cs.pressuregrid(50.0, 1e5, np_)


def _column(cs, lines, ctx, which, nu, absorbers, np_, nlob, T=None, extra_gases=()):
    """absorbers: callables gas -> absorber (CIATables need no gas, a Continuum does)"""
    g = _gas(cs, lines, which, nu)
    return cs.Column(_pgrid(cs, np_), CR.G, CR.profile(np_) if T is None else T, 0.044, 0.0, 0.0, g, *extra_gases, *[a(g) for a in absorbers],
                     core=cs.Discretized(4, nlob), ctx=ctx, _warn=False)


def _run(cs, lines, which, nu, absorbers, np_, nlob, tune, T=None, extra_gases=(), sigma_only=False):
    ctx = cs.Context(0)
    try:
        for k, v in tune:
            ctx.set_tuning(k, v)
        col = _column(cs, lines, ctx, which, nu, absorbers, np_, nlob, T, extra_gases)
        if sigma_only:
            col.sigma_run()
            col.sync()
            return dict(sigma=col.sigma_nodes(), col=col)
        col.run()
        r = B._outputs(col)
        r["sigma"], r["col"] = col.sigma_nodes(), col
        return r
    finally:
        ctx.close()


def _tables(cs, data, **kw):
    return lambda gas: cs.CIATables(data, radiation=True, **kw)


def _st(col):
    return dict(Tk=col.Tk, Pk=col.Pk)


def _reference(O, col, sig):
    with np.errstate(invalid="ignore"):
        return O.fluxes_discretized(col.nu, col.P, col.g, col.core.nlobatto, col.Tn, col.mun, col.Tlev, [g.sl for g in col.gases],
                                    ["voigt"] * len(col.gases), list(col.cuts), col.conc, sigma_extra=sig, nstream=col.core.nstream,
                                    theta_s=col.theta_s)


def _check(cs, r, sig, ref, bands, nlob, label, fluxes=True, tau=True):
    """tests/test_gpu_cia_bands.py's _check with continuum_ref.bound in place of tabulated_ref.cia_bound"""
    bs, bt = CR.bound(bands), CR.bound(bands, nlob)
    assert bt < 1e-12
    assert not np.isnan(sig).any()
    rs = B._ratio(r["sigma"], sig, bs)
    rt = B._ratio(r["tau"], ref["tau"], bt) if tau else 0.0
    print(f"  {label}: sigma err/bound {rs:.3f}  tau err/bound {rt:.3f}")
    assert rs <= 4.0 and rt <= 4.0, (label, rs, rt)
    if fluxes and tau:
        sm = max(ref["Mup"].max(), ref["Mdn"].max())
        amp = B._amp(cs, r["col"].nu, r["col"].Tlev, ref["tau"])
        for k in ("Mup", "Mdn"):
            assert np.all(np.abs(r[k] - ref[k]) < 1e-11 * sm + amp[None, :]), (label, k)
        for k in ("Fup", "Fdn"):
            assert np.max(np.abs(r[k] - ref[k])) < 1e-11 * ref["Fup"].max(), (label, k)


def _forms(cs, O, lines, which, nu, absorbers, objs, flagged, np_, nlob, forms=FORMS, extra_gases=(), T=None):
    """one absorber set through the flux forms: each against the reference, then against the first"""
    bands = sum((d for d, _, _ in objs), [])
    res, sig, ref = [], None, None
    for name, tune, form in forms:
        r = _run(cs, lines, which, nu, absorbers, np_, nlob, tune, T=T, extra_gases=extra_gases)
        B._is(r, form, tune)
        if sig is None:
            sig = CR.plane(objs, nu, _st(r["col"]), flagged)
            ref = _reference(O, r["col"], sig)
            B._above_floor(ref)
        _check(cs, r, sig, ref, bands, nlob, f"{which} {name}")
        res.append(r)
    bt = CR.bound(bands, nlob)
    for r in res[1:]:
        assert B._ratio(r["tau"], res[0]["tau"], bt) <= 4.0
        amp = B._amp(cs, nu, r["col"].Tlev, ref["tau"])
        sm = max(ref["Mup"].max(), ref["Mdn"].max())
        assert np.all(np.abs(r["Mup"] - res[0]["Mup"]) < 1e-11 * sm + amp[None, :])
    return res, sig, ref


# ---- 1: the plane form ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,nnu,np_,nlob", [("high", 200, 6, 3), ("low", 257, 5, 2)])
def test_sigma_plane(cs, lines, which, nnu, np_, nlob):
    """cs_column_sigma_run (k_cia<true>) against the reference on both grids; level temperatures on and between table knots.  Without
    the flag's arithmetic the plane is off by the factor R: 1.4e4 on the high grid, 7e-4 .. 15 on the low one"""
    nu = CR.grid(which, nnu)
    data = CR.bands_for(which, nu, symbol=SYMBOL[which])
    r = _run(cs, lines, which, nu, [_tables(cs, data)], np_, nlob, (), sigma_only=True)
    col = r["col"]
    assert all(t in col.Tk for t in (220.0, 260.0, 300.0))
    sig = CR.plane([(data, X1, X1)], nu, _st(col))
    assert (sig > 0).mean() > 0.5
    rs = B._ratio(r["sigma"], sig, CR.bound(data))
    print(f"  {which}: sigma err/bound {rs:.3f}")
    assert rs <= 4.0, rs


# ---- 2: the flux forms ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,nnu,np_,nlob", [("high", 320, 9, 3), ("low", 192, 6, 2), ("low", 257, 7, 3)])
def test_flux_forms(cs, O, lines, which, nnu, np_, nlob):
    nu = CR.grid(which, nnu)
    data = CR.bands_for(which, nu, symbol=SYMBOL[which])
    _forms(cs, O, lines, which, nu, [_tables(cs, data)], [(data, X1, X1)], None, np_, nlob)


# ---- 3: a flagged object beside an unflagged one ---------------------------------------------------------------------------------

@pytest.mark.parametrize("flagged_first", [True, False])
def test_flagged_beside_unflagged(cs, O, lines, flagged_first):
    """two objects whose bands overlap on tile 1 (points 64 .. 127), one flagged: R multiplies that object's band sum only, whichever comes
    first.  The unflagged one is raised to the flagged one's size, so that R applied per column (or to the wrong object) is off by orders"""
    nu = CR.grid("high", 200)
    a = CR.shifted(R.band(nu[40], nu[150], 17, R.TS, 1) + R.band(nu[64], nu[127], 6, R.TS, 2), CR.LEVEL["high"])
    b = R.band(nu[60] - 0.01, nu[199], 29, R.TS, 5, "CO2-CH4") + R.band(nu[70], nu[120], 4, R.TS, 6, "CO2-CH4")
    assert min(R.tile_overlaps(a, nu)[1], R.tile_overlaps(b, nu)[1]) == 2
    x_ch4 = 0.05
    ch4 = cs.DirectGas(lines("CH4"), x_ch4, nu)
    A = (lambda gas: cs.CIATables(a, radiation=True)), (a, X1, X1), True
    Bq = (lambda gas: cs.CIATables(b)), (b, X1, x_ch4), False
    order = [A, Bq] if flagged_first else [Bq, A]
    res, sig, _ = _forms(cs, O, lines, "high", nu, [o[0] for o in order], [o[1] for o in order], [o[2] for o in order], 7, 3, extra_gases=(ch4,))
    st = _st(res[0]["col"])
    one, two = CR.plane([A[1]], nu, st), CR.plane([Bq[1]], nu, st, [False])
    both = (one[3] > 0) & (two[3] > 0)
    assert both[64:128].all() and 1e-2 < np.median(one[3, both] / two[3, both]) < 1e2


# ---- 4: the same absorber through sigma_extra --------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["high", "low"])
def test_route_equivalence(cs, lines, which):
    """the flagged object on the device against the host functor (CIATables.__call__, which applies R too) handed over as a function
    absorber: both are double evaluations of one formula, each held to 4 x bound of the exact value, so they differ by at most 8 x bound;
    band fluxes to 1e-11 of the largest"""
    nu = CR.grid(which, 192)
    data = CR.bands_for(which, nu, symbol=SYMBOL[which])
    dev = _run(cs, lines, which, nu, [_tables(cs, data)], 6, 3, ())
    x = cs.CIATables(data, radiation=True)

    def host(gas):
        pair = cs.CIA(x, [gas])
        return lambda v, T, P: np.array([pair(float(t), T, P) for t in np.atleast_1d(v)])
    ext = _run(cs, lines, which, nu, [host], 6, 3, ())
    assert ext["col"].sigma_extra is not None and dev["col"].sigma_extra is None
    rs = B._ratio(dev["sigma"], ext["sigma"], CR.bound(data))
    e = max(np.max(np.abs(dev[k] - ext[k])) for k in ("Fup", "Fdn")) / ext["Fup"].max()
    print(f"  {which}: device against sigma_extra: sigma diff/bound {rs:.3f}  flux {e:.2e}")
    assert rs <= 8.0 and e < 1e-11


# ---- 5: update ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tune,form", [(B.SCAN, 3), (B.CHUNK, 2), (B.SEP, 0)])
def test_update_to_a_far_profile(cs, O, lines, tune, form):
    """Column.update to a profile 60 K away: R follows the new node temperatures -- equal to a fresh column there, and to the reference"""
    which, np_, nlob = "low", 6, 3
    nu = CR.grid(which, 200)
    data = CR.bands_for(which, nu, seed=1, symbol=SYMBOL[which])
    T2 = CR.profile(np_, 250.0, 338.0)[::-1].copy()
    ctx = cs.Context(0)
    try:
        for k, v in tune:
            ctx.set_tuning(k, v)
        col = _column(cs, lines, ctx, which, nu, [_tables(cs, data)], np_, nlob, T=np.full(np_, 190.0))
        col.run()
        a = B._outputs(col)
        col.update(T2)
        col.run()
        b = B._outputs(col)
        b["sigma"], b["col"] = col.sigma_nodes(), col
        B._is(b, form, tune)
        assert not np.array_equal(a["tau"], b["tau"])
        sig = CR.plane([(data, X1, X1)], nu, _st(col))
        ref = _reference(O, col, sig)
        B._above_floor(ref)
        _check(cs, b, sig, ref, data, nlob, "updated")
    finally:
        ctx.close()
    f = _run(cs, lines, which, nu, [_tables(cs, data)], np_, nlob, tune, T=T2)
    _check(cs, f, sig, ref, data, nlob, "fresh")
    for k in ("tau", "Mup", "Mdn", "Fup", "Fdn"):
        assert np.array_equal(b[k], f[k]), k


# ---- 6: batches ---------------------------------------------------------------------------------------------------------------------

def test_run_batch(cs, O, lines):
    """cs_column_batch forms R at B K states through cia_states: three profiles against three single runs and the reference"""
    which, np_, nlob = "low", 7, 3
    nu = CR.grid(which, 200)
    data = CR.bands_for(which, nu, seed=1, symbol=SYMBOL[which])
    Ts = [CR.profile(np_), CR.profile(np_, 250.0, 338.0)[::-1].copy(), np.full(np_, 231.0) + 3.0 * np.arange(np_)]
    ctx = cs.Context(0)
    try:
        col = _column(cs, lines, ctx, which, nu, [_tables(cs, data)], np_, nlob)
        Fup, Fdn = col.run_batch(Ts)
    finally:
        ctx.close()
    for b, T in enumerate(Ts):
        one = _run(cs, lines, which, nu, [_tables(cs, data)], np_, nlob, (), T=T)
        sig = CR.plane([(data, X1, X1)], nu, _st(one["col"]))
        ref = _reference(O, one["col"], sig)
        B._above_floor(ref)
        e1 = max(np.max(np.abs(Fup[b] - one["Fup"])), np.max(np.abs(Fdn[b] - one["Fdn"]))) / ref["Fup"].max()
        e2 = max(np.max(np.abs(Fup[b] - ref["Fup"])), np.max(np.abs(Fdn[b] - ref["Fdn"]))) / ref["Fup"].max()
        print(f"  profile {b}: flux err against a single run {e1:.2e}, against the reference {e2:.2e}")
        assert e1 < 1e-11 and e2 < 1e-11, (b, e1, e2)


# ---- 7: the accelerated absorber ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["high", "low"])
def test_accelerated_absorber(cs, lines, which):
    """cs_accel_store over a flagged object: the stored knot values are ln of the reference, to 4 x bound / |ln sigma| + one rounding of ln"""
    nu = CR.grid(which, 192)
    data = CR.bands_for(which, nu, seed=1, symbol=SYMBOL[which])
    Pk = _pgrid(cs, 6)
    Tk = CR.profile(6)
    ctx = cs.Context(0)
    try:
        g = _gas(cs, lines, which, nu)
        A = cs.AcceleratedAbsorber(Tk, Pk, g, cs.CIATables(data, radiation=True), ctx=ctx)
        L = np.zeros((len(Pk), len(nu)))
        cs.check(cs.lib().cs_accel_fetch(ctx.handle, A.slot, len(nu), len(Pk), cs.dptr(L)))
    finally:
        ctx.close()
    sig = CR.plane([(data, X1, X1)], nu, dict(Tk=A.T, Pk=A.P))
    ok = sig > 0
    assert ok.mean() > 0.5
    err = np.abs(L[ok] - np.log(sig[ok]))
    tol = 4.0 * CR.bound(data) + 2.0 * R.U * np.abs(np.log(sig[ok]))
    print(f"  {which}: knot values err/tolerance {np.max(err / tol):.3f}")
    assert np.all(err <= tol)


# ---- 8: end to end ----------------------------------------------------------------------------------------------------------------------

def _coefficients(nu_s, T):
    """made-up continuum coefficients [cm^2 molecule^-1 per cm^-1]: smooth, falling with wavenumber and temperature"""
    return 2e-22 * np.exp(-nu_s / 400.0) * (296.0 / T) ** 4.0 * (1.0 + 0.2 * np.sin(nu_s / 30.0))


def test_end_to_end_fluxes(cs, lines):
    """H2O voigtCKD lines + a self and a foreign Continuum through fluxes(), against the same column whose continua are host functions
    (sigma_extra); a temperature outside the self table is refused"""
    nu = np.linspace(1400.0, 1500.0, 257)
    P, T = _pgrid(cs, 8), CR.profile(8, 210.0, 295.0)
    x = lambda T_, P_: 0.01 * (P_ / 1e5)
    nu_s = np.linspace(1390.0, 1510.0, 25)
    self_data = [dict(nu=nu_s, T=t, C=_coefficients(nu_s, t)) for t in (200.0, 260.0, 296.0, 330.0)]
    foreign_data = {296.0: 3e-3 * _coefficients(nu_s, 296.0)}
    out = {}
    for route in ("device", "host"):
        ctx = cs.Context(0)
        try:
            h2o = cs.DirectGas(lines("H2O"), x, nu, shape="voigtCKD")
            cs_, cf = cs.Continuum(self_data, h2o, "self"), cs.Continuum(foreign_data, h2o, "foreign", nu=nu_s)
            assert (cs_.x.radiation, cs_.x.singles, cf.x.singles, cf.x.extrapolate) == (True, False, True, False)
            members = (cs_, cf) if route == "device" else tuple((lambda c: lambda v, T_, P_: np.array([c(float(t), T_, P_) for t in np.atleast_1d(v)]))(c)
                                                                for c in (cs_, cf))
            out[route] = cs.fluxes(P, CR.G, T, 0.029, 0.0, 0.0, h2o, *members, core=cs.Discretized(4, 3), theta_s=0.0, ctx=ctx)
            if route == "device":
                lines_only = cs.fluxes(P, CR.G, T, 0.029, 0.0, 0.0, h2o, core=cs.Discretized(4, 3), theta_s=0.0, ctx=ctx)
                with pytest.raises(ValueError, match="outside the table's range"):
                    cs.fluxes(P, CR.G, np.full(8, 340.0), 0.029, 0.0, 0.0, h2o, cs_, core=cs.Discretized(4, 3), theta_s=0.0, ctx=ctx)
        finally:
            ctx.close()
    top = out["host"][0].max()
    e = max(np.max(np.abs(out["device"][i] - out["host"][i])) for i in (0, 1)) / top
    moved = np.max(np.abs(out["device"][0] - lines_only[0])) / top
    print(f"  device against sigma_extra: {e:.2e} of the largest flux; the continua move the fluxes by {moved:.2e}")
    assert e < 1e-11 and moved > 1e-4


def test_unknown_flag_refused(cs, lines):
    nu = CR.grid("high", 96)
    data = CR.bands_for("high", nu)
    ctx = cs.Context(0)
    try:
        col = _column(cs, lines, ctx, "high", nu, [_tables(cs, data)], 5, 2)
        slots = np.array([ctx.cia_slot(col.U.cia[0].x)], dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        p = cs.dptr(np.ascontiguousarray(col.cia_P1.ravel()))
        for fl, rc in ((8, -1), (12, -1), (1 << 30, -1), (7, 0), (4, 0)):
            assert cs.lib().cs_column_set_cia(ctx.handle, 1, ip(slots), ip(np.array([fl], dtype=np.int32)), p, p) == rc, fl
    finally:
        ctx.close()
