"""References and synthetic inputs for CIA objects flagged CS_CIA_RADIATION (include/clearsky_hip.h), shared by tests/test_continuum.py
(host) and tests/test_gpu_continuum.py (device).  The reference of a flagged object is tabulated_ref.cia_sigma x R with
R(nu, T) = nu tanh(c2 nu / 2T) in mpmath at 40 digits; optical depths and fluxes come from the oracle fed that plane as sigma_extra.

Two grids: HIGH, tabulated_ref's grid above the CO2 fixture's last line + 25 cm^-1 (tanh is 1 to rounding there, R = nu), and LOW,
0.5 .. 80 cm^-1 under a synthetic H2O line table whose lines all lie above 5000 cm^-1 (tanh in its small-argument regime, R between
7e-4 and 15 cm^-1: a (1 - e) / (1 + e) form loses digits there).  The synthetic ln k of tabulated_ref sits near -100; `shifted` moves a
data set's level so that a good share of the layer optical depths lies above the 1e-6 floor on either grid (checked on the host by
tests/test_continuum.py with the reference alone, and again by every device case).
"""
import mpmath as mp
import numpy as np

import tabulated_ref as R

from clearsky_jl_amd import constants as C_

mp.mp.dps = 40
U = R.U
C2 = 100 * mp.mpf(C_.h) * mp.mpf(C_.c) / mp.mpf(C_.k)
G = 9.8
LEVEL = {"high": -9.0, "low": 4.0}          # added to tabulated_ref's ln k (near -100): R is ~1.4e4 cm^-1 on HIGH, 7e-4 .. 15 on LOW


def radiation(nu, T):
    """R(nu, T) as mpf, one per wavenumber"""
    T = mp.mpf(float(T))
    return [mp.mpf(float(v)) * mp.tanh(C2 * mp.mpf(float(v)) / (2 * T)) for v in np.atleast_1d(nu)]


def sigma(bands, nu, T, Pa, P1, P2, extrapolate=False, singles=False):
    """the flagged object's cross-section at one state: cia_sigma x R, NaN where cia_sigma has it"""
    s = R.cia_sigma(bands, nu, T, Pa, P1, P2, extrapolate, singles)
    return np.array([np.nan if np.isnan(a) else float(mp.mpf(float(a)) * r) for a, r in zip(s, radiation(nu, T))])


def bound(bands, nlobatto=None):
    """tabulated_ref.cia_bound + 8 U: the three roundings of the argument, the tanh, and the two products, with the condition number of
    x tanh x in x at most 2.  Tests assert 4 x this."""
    return R.cia_bound(bands, nlobatto) + 8.0 * U


def shifted(bands, dln):
    """the same bands with ln k moved by dln"""
    return [dict(d, k=np.asarray(d["k"], float) * np.exp(dln)) for d in bands]


def grid(which, n):
    if which == "high":
        return R.grid(n)
    return np.linspace(0.5, 80.0, n)


def bands_for(which, nu, seed=0, symbol="CO2-CO2"):
    """three bands over the grid: a wide one on all five temperatures, one over tiles 1.. on three, a short one on two samples; bands 0
    and 1 overlap from point 64 on"""
    n = len(nu)
    d = (R.band(nu[0] - 0.25 * (nu[1] - nu[0]), nu[min(n - 1, 150)], 23, R.TS, 1 + seed, symbol)
         + R.band(nu[64], nu[-1] + 0.3, 31, R.TS[1:4] if seed == 0 else R.TS, 2 + seed, symbol)
         + R.band(nu[10], nu[30], 2, R.TS, 3 + seed, symbol))
    return shifted(d, LEVEL[which])


def profile(np_, lo=185.0, hi=335.0):
    """level temperatures inside every band's range of bands_for (a continuum is never extrapolated), with levels exactly on the knots
    220, 260 and 300 K and the others between knots"""
    T = np.linspace(lo, hi, np_)
    for knot in (220.0, 260.0, 300.0):
        T[int(np.argmin(np.abs(T - knot)))] = knot
    return T


def low_lines(cs):
    """a synthetic H2O table with every line above 5000 cm^-1: nothing within 25 cm^-1 of the LOW grid"""
    sl = cs.SpectralLines.synthetic(1, 40, 5, 5000.0, 5400.0)
    assert sl.nu.min() > 5000.0
    return sl


def states(cs, P, T, nlob, mu=0.044):
    """node temperatures, pressures and level temperatures of a column on the host, as Column forms them"""
    fT, fmu = cs.core.formprofile(P, T), cs.core.formprofile(P, mu)
    Tn, mun = cs.core.lobattoevaluations(P, fT, fmu, nlob)
    return dict(Tn=Tn, mun=mun, Tk=cs.core.nodevalues(Tn, nlob), Pk=cs.core.nodepressures(P, nlob), Tlev=np.array([fT(p) for p in P]))


def reference(O, cs, sl, nu, P, T, nlob, sig, conc=0.9, nstream=4, theta_s=0.0):
    """the oracle's depths, sweeps and band fluxes over a line gas that contributes nothing on the grid plus the plane `sig`"""
    st = states(cs, P, T, nlob)
    K = len(st["Tk"])
    with np.errstate(invalid="ignore"):
        return O.fluxes_discretized(nu, P, G, nlob, st["Tn"], st["mun"], st["Tlev"], [sl], ["voigt"], [25.0], np.full((1, K), conc, order="F"),
                                    sigma_extra=sig, nstream=nstream, theta_s=theta_s)


def plane(objs, nu, st, flagged=None):
    """sum over objects (bands, x1, x2): partial pressures P x1, P x2 at every node; flagged[i] False leaves R off object i"""
    out = np.zeros((len(st["Tk"]), len(nu)))
    for i, (d, x1, x2) in enumerate(objs):
        f = sigma if (flagged is None or flagged[i]) else R.cia_sigma
        for k, (T, P) in enumerate(zip(st["Tk"], st["Pk"])):
            out[k] += f(d, nu, T, P, P * x1, P * x2)
    return out
