"""Arbitrary-precision references of the three tabulated absorbers and synthetic inputs for them, shared by tests/test_tabulated_ref.py
(host), tests/test_gpu_cia_bands.py and tests/test_gpu_table_eval.py (device).  Everything is restated from the formulas of the
reference's sources (line numbers below) in mpmath at 40 digits and returned as doubles; the knot values themselves -- ln k of a CIA
band, ln sigma of a table -- are the doubles the library is given, so only the arithmetic between knots and result is exact here.
One exception, in table_sigma: for tables of more than 4096 values (wavenumbers x knots) the M-term sum is taken with the exact weights
rounded to 64-bit significands in numpy's long double (an error of (M + 1) 2^-64 sum |Z||W|, 1/2000 of the bound the sum is held to)
and only the exponential in mpmath; where long double is no wider than double the full mpmath sum runs for every size.

  cia_k / cia_sigma   the CIATables functor (collision_induced_absorption.jl:251-276) and cia(k, T, Pa, P1, P2) (:295-303)
  table_sigma         OpacityTable's functor exp(Phi(T, ln P)) (gases.jl:80,85): the interpolating polynomial through the knots
  accel_sigma         AcceleratedAbsorber's exp(phi_i(ln P)) (absorbers.jl:195,203): linear in ln P, end cells extrapolated
  cia_bound, table_bound, accel_bound   the derived tolerances (docstrings)
  band, single, SETS  synthetic CIA data in the form readcia returns
"""
import math

import mpmath as mp
import numpy as np

from clearsky_jl_amd import constants as C_

mp.mp.dps = 40
U = 2.0 ** -53                       # unit roundoff of a double; one ulp = 2 U

# ---- collision-induced absorption ---------------------------------------------------------------------------------------------


def _groups(bands):
    """CIATables (:161-208): the dicts grouped by their (numin, numax) range, ranges in ascending order of numin; one dict = a
    single-temperature range (ln k with k <= 0 -> 0, :186-188), several = a grid sorted by T (k <= 0 -> floatmin, :205-207)"""
    ranges = sorted(set((d["numin"], d["numax"]) for d in bands), key=lambda r: r[0])
    out = []
    for lo, hi in ranges:
        sel = [d for d in bands if math.isclose(d["numin"], lo) and math.isclose(d["numax"], hi)]
        if len(sel) == 1:
            k = np.array(sel[0]["k"], float)
            k[k <= 0.0] = 0.0
            with np.errstate(divide="ignore"):
                out.append((np.asarray(sel[0]["nu"], float), None, np.log(k)[None, :]))
        else:
            sel = sorted(sel, key=lambda d: d["T"])
            k = np.array([d["k"] for d in sel], float)
            k[k <= 0.0] = np.finfo(float).tiny
            out.append((np.asarray(sel[0]["nu"], float), np.array([d["T"] for d in sel], float), np.log(k)))
    return out


def _cells(g, v):
    """cell i with g[i] <= v < g[i+1], the last cell for v == g[-1] (BasicInterpolators' findcell: clamped to 0 .. n-2)"""
    return np.clip(np.searchsorted(g, v, side="right") - 1, 0, len(g) - 2)


def _linear_ieee(v, xa, xb, ya, yb):
    """phi(nu) = (nu - x_i) (y_{i+1} - y_i) / (x_{i+1} - x_i) + y_i  (LinearInterpolator, :188,271) where samples may be ln 0 = -inf.
    mpmath has no IEEE infinities in products, so the expression is evaluated by its IEEE rules, read off the expression above:
      y_i = -inf                 : y_{i+1} - y_i is +inf (or NaN when both are -inf); (nu - x_i) * that is +inf or 0 * inf = NaN;
                                   adding y_i = -inf gives NaN in every case -> NaN on the whole cell, both ends included
      y_i finite, y_{i+1} = -inf : the slope is -inf; at nu == x_i it is 0 * -inf = NaN, elsewhere -inf, and exp(-inf) = 0
    Returns exp(phi) as an mpf, or None for NaN."""
    if ya == -np.inf:
        return None
    if yb == -np.inf:
        return None if v == xa else mp.mpf(0)
    v, xa, xb, ya, yb = (mp.mpf(float(t)) for t in (v, xa, xb, ya, yb))
    return mp.exp((v - xa) * (yb - ya) / (xb - xa) + ya)


def cia_k(bands, nu, T, extrapolate=False, singles=False):
    """tables(nu, T) (:251-276) for a vector of wavenumbers -> (k as mpf or None (NaN) per wavenumber)"""
    nu = np.atleast_1d(np.asarray(nu, float))
    tot = [mp.mpf(0)] * len(nu)
    for g, Tg, ln in _groups(bands):
        inside = np.nonzero((g[0] <= nu) & (nu <= g[-1]))[0]          # Phi.G.xa <= nu <= Phi.G.xb, inclusive (:255, :270)
        if not len(inside):
            continue
        cells = _cells(g, nu[inside])
        if Tg is None:
            if not singles:                                           # :267
                continue
            for n, i in zip(inside, cells):
                e = _linear_ieee(nu[n], g[i], g[i + 1], ln[0, i], ln[0, i + 1])
                tot[n] = None if (e is None or tot[n] is None) else tot[n] + e
            continue
        if Tg[0] <= T <= Tg[-1]:                                      # :258
            Te = T
        elif extrapolate:                                             # :261-263: flat beyond the temperature ends
            Te = Tg[-1] if T > Tg[-1] else Tg[0]
        else:
            continue
        j = int(_cells(Tg, np.array([Te]))[0])
        y = (mp.mpf(float(Te)) - mp.mpf(float(Tg[j]))) / (mp.mpf(float(Tg[j + 1])) - mp.mpf(float(Tg[j])))
        for n, i in zip(inside, cells):
            x = (mp.mpf(float(nu[n])) - mp.mpf(float(g[i]))) / (mp.mpf(float(g[i + 1])) - mp.mpf(float(g[i])))
            z = [mp.mpf(float(ln[a, b])) for a, b in ((j, i), (j, i + 1), (j + 1, i), (j + 1, i + 1))]
            e = mp.exp((1 - x) * (1 - y) * z[0] + x * (1 - y) * z[1] + (1 - x) * y * z[2] + x * y * z[3])     # bilinear in ln k (:207)
            if tot[n] is not None:
                tot[n] = tot[n] + e
    return tot


def cia_sigma(bands, nu, T, Pa, P1, P2, extrapolate=False, singles=False):
    """cia(nu, tables, T, Pa, P1, P2) (:318-323) = (k Lo^2) rho1 rho2 / rhoa (:295-303) -> doubles, NaN where the reference has it"""
    T_, Pa_, P1_, P2_ = (mp.mpf(float(t)) for t in (T, Pa, P1, P2))
    rho1 = (P1_ / mp.mpf(C_.atm)) * (mp.mpf(C_.T0) / T_)
    rho2 = (P2_ / mp.mpf(C_.atm)) * (mp.mpf(C_.T0) / T_)
    rhoa = mp.mpf("1e-6") * Pa_ / (mp.mpf(C_.k) * T_)
    f = mp.mpf(C_.Lo2) * rho1 * rho2 / rhoa
    return np.array([np.nan if k is None else float(k * f) for k in cia_k(bands, nu, T, extrapolate, singles)])


def max_abs_lnk(bands):
    """max |ln k| over the finite samples of a data set (floatmin-clamped grids included)"""
    m = 0.0
    for _, _, ln in _groups(bands):
        f = ln[np.isfinite(ln)]
        m = max(m, float(np.max(np.abs(f)))) if f.size else m
    return m


def cia_bound(bands, nlobatto=None):
    """Relative error a double evaluation of sigma (nlobatto=None) or of a layer's optical depth may have against the exact value:
    the exponent is a bilinear form of four samples -- at most 12 roundings on terms bounded by max |ln k| -- so |d ln k| <= 12 U max|ln k|;
    the device exponential is good to 2 ulp = 4 U (tests/test_gpu_kat.py); Lo^2 rho1 rho2 / rhoa is 4 more roundings; a layer's optical
    depth is a Lobatto sum of nlobatto such terms and a scale: nlobatto + 2 more.  Tests assert 4 x this."""
    return (12.0 * max_abs_lnk(bands) + 4.0 + 4.0 + (0.0 if nlobatto is None else nlobatto + 2.0)) * U


# ---- synthetic CIA data ------------------------------------------------------------------------------------------------------------

def _lnk(nu, T, seed):
    """a smooth ln k in [-110, -90] that is neither linear in nu nor in T, different for every band"""
    nu = np.asarray(nu, float)
    return -100.0 + 6.0 * np.sin(0.37 * nu + seed) + 3.0 * np.cos(0.011 * T * (1 + 0.1 * seed)) + 0.9 * np.sin(0.05 * (nu - nu[0]) * (T / 250.0))


def band(lo, hi, nb, Ts, seed, symbol="CO2-CO2", nu=None):
    """a grid band on nb samples of [lo, hi] (or the given samples) at the temperatures Ts: one readcia dict per temperature"""
    nu = np.linspace(lo, hi, nb) if nu is None else np.asarray(nu, float)
    return [dict(symbol=symbol, numin=float(nu[0]), numax=float(nu[-1]), npts=len(nu), T=float(T), nu=nu.copy(), k=np.exp(_lnk(nu, T, seed)))
            for T in Ts]


def single(lo, hi, nb, T, seed, zeros=(), symbol="CO2-CO2"):
    """a single-temperature range with k = 0 at the sample indices `zeros`"""
    nu = np.linspace(lo, hi, nb)
    k = np.exp(_lnk(nu, T, seed))
    k[list(zeros)] = 0.0
    return [dict(symbol=symbol, numin=float(nu[0]), numax=float(nu[-1]), npts=nb, T=float(T), nu=nu, k=k)]


TS = (180.0, 220.0, 260.0, 300.0, 340.0)
NU0 = 14100.0                      # above the CO2 fixture's last line + 25 cm^-1: a CO2 line gas contributes nothing here


def grid(n, step=0.25):
    return NU0 + step * np.arange(n)


def overlap_set(n, symbol="CO2-CO2"):
    """n grid bands that all cover tile 1 (points 64..127) of grid(200), each with its own ends, sample count and temperatures; band 0 has
    two samples, the last of overlap_set(4) has 300 (> 256: second block of the temperature pass).  Tile 0 sees fewer bands."""
    a, b = NU0 + 64 * 0.25, NU0 + 127 * 0.25
    out = []
    nbs = (2, 7, 40, 300, 11, 5)
    for q in range(n):
        out += band(a - 3.3 * q - 0.1, b + 2.1 * q + 0.07, nbs[q], TS[: 2 + q % 4] if q else TS, seed=q + 1, symbol=symbol)
    return out


def many_bands(n, symbol="CO2-CO2"):
    """n narrow bands side by side (at most two on a tile of grid(200)... each 3.1 cm^-1 wide, 2 cm^-1 apart)"""
    return sum((band(NU0 - 1.0 + 2.0 * q, NU0 + 2.1 + 2.0 * q, 4 + q % 5, TS[q % 3: q % 3 + 2 + q % 2], seed=q + 1, symbol=symbol) for q in range(n)), [])


def ends_set(nu):
    """band ends against the grid nu (>= 130 points, two tiles and more): ends exactly on grid points, on the first and last point of
    tile 1, strictly between two neighbouring points, between the last point of tile 0 and the first of tile 1, wider than the grid, and
    ends one ulp inside grid points (those points get nothing)"""
    up, dn = (lambda x: float(np.nextafter(x, np.inf))), (lambda x: float(np.nextafter(x, -np.inf)))
    mid = lambda i, f: float(nu[i] + f * (nu[i + 1] - nu[i]))
    return (band(nu[5], nu[20], 9, TS, 1)                              # first / last sample = a grid point
            + band(nu[64], nu[127], 6, TS[:3], 2)                      # exactly tile 1
            + band(mid(30, 0.2), mid(30, 0.7), 3, TS, 3)               # between two neighbouring points: reaches tile 0, holds no point
            + band(mid(63, 0.3), mid(63, 0.6), 4, TS, 4)               # between two tiles: reaches neither
            + band(nu[0] - 7.0, nu[-1] + 9.0, 33, TS, 5)               # wider than the grid
            + band(up(nu[40]), dn(nu[50]), 5, TS[1:], 6))              # points 40 and 50 are one ulp outside


def singles_set(nu):
    """a grid band under two single-temperature ranges with k = 0 samples: isolated (index 3), two in a row (6, 7), at a range end (0 of
    the second range and its last)"""
    return (band(nu[0] - 1.0, nu[-1] + 1.0, 12, TS, 1)
            + single(nu[10], nu[60], 11, 250.0, 2, zeros=(3, 6, 7))
            + single(float(nu[70]) + 0.01, float(nu[120]), 9, 250.0, 3, zeros=(0, 8)))


def tile_overlaps(bands, nu):
    """bands of one object reaching each 64-point tile of the grid: first sample <= the tile's last point and last sample >= its first"""
    g = _groups(bands)
    nu = np.asarray(nu, float)
    return [sum(1 for b, _, _ in g if b[0] <= nu[min(t + 63, len(nu) - 1)] and b[-1] >= nu[t]) for t in range(0, len(nu), 64)]


# ---- opacity tables -------------------------------------------------------------------------------------------------------------

def _lagrange(x, v):
    """Lagrange basis l_i(v) = prod_{j != i} (v - x_j) / (x_i - x_j) on the knots x (doubles), in mpmath"""
    x = [mp.mpf(float(t)) for t in x]
    out = []
    for i in range(len(x)):
        p = mp.mpf(1)
        for j in range(len(x)):
            if j != i:
                p *= (v - x[j]) / (x[i] - x[j])
        out.append(p)
    return out


def _ln(P, Pgrid, lnP):
    """ln P exactly -- or the knot itself where P is one of the knot pressures (the knots are the doubles log(P_j))"""
    hit = np.nonzero(np.asarray(Pgrid, float) == float(P))[0]
    return mp.mpf(float(lnP[hit[0]])) if len(hit) else mp.log(mp.mpf(float(P)))


def table_sigma(Z, Tgrid, Pgrid, T, P):
    """exp(Phi(T, ln P)) for every wavenumber, Z[nnu, nT, nP] = ln sigma on the knots: the unique polynomial of degree (nT-1, nP-1) in
    (T, ln P) through the knot values (BichebyshevInterpolator, gases.jl:80,85), as a plain Lagrange product.  The ln P knots are the
    doubles log(P_j) the library forms; ln P of the point is exact, clamped to the knots' ends (the library accepts 1e-12 beyond them).
    Returns (sigma[nnu], A[nnu]) with A = sum_m |Z_m| |W_m| for the exact weights W."""
    Z = np.asarray(Z, float)
    lnP = np.log(np.asarray(Pgrid, float))
    x = _ln(P, Pgrid, lnP)
    x = min(max(x, mp.mpf(float(lnP[0]))), mp.mpf(float(lnP[-1])))
    a, b = _lagrange(Tgrid, mp.mpf(float(T))), _lagrange(lnP, x)
    W = [[a[i] * b[j] for j in range(len(b))] for i in range(len(a))]
    Wf = np.array([[float(abs(w)) for w in r] for r in W])
    A = np.sum(np.abs(Z) * Wf[None], axis=(1, 2))
    if Z.shape[0] * Wf.size <= 4096 or np.finfo(np.longdouble).nmant < 63:
        s = [sum((mp.mpf(float(Z[n, i, j])) * W[i][j] for i in range(len(a)) for j in range(len(b))), mp.mpf(0)) for n in range(Z.shape[0])]
        return np.array([float(mp.exp(t)) for t in s]), A
    # long tables: the exact weights rounded to 64-bit significands, the M-term sum in that arithmetic -- (M + 1) 2^-64 A, 1/2000 of the
    # bound the sum is held to -- and the exponential of the sum (split into two doubles) in mpmath again
    hi = np.array([[float(w) for w in r] for r in W])
    lo = np.array([[float(w - mp.mpf(h)) for w, h in zip(r, hr)] for r, hr in zip(W, hi)])
    Wl = hi.astype(np.longdouble) + lo.astype(np.longdouble)
    s = np.sum(Z.astype(np.longdouble) * Wl[None], axis=(1, 2))
    s0 = s.astype(float)
    s1 = (s - s0.astype(np.longdouble)).astype(float)
    return np.array([float(mp.exp(mp.mpf(float(u)) + mp.mpf(float(v)))) for u, v in zip(s0, s1)]), A


def table_bound(nT, nP, A):
    """|d exponent| <= (M + 4 (nT + nP) + 8) U A for the M = nT nP term dot product with weights that are products of two barycentric
    quotients; relative error of sigma <= that + 4 ulp"""
    return (nT * nP + 4.0 * (nT + nP) + 8.0) * U * np.asarray(A) + 8.0 * U


def table_values(nu, nT, nP, lo=-120.0, hi=-40.0):
    """Z[i, iT, iP] = f(nu_i) + g(iT) + h(iP) + a small cross term, in [lo, hi], with g != h and every knot distinct: a transposed index,
    a dropped node or a shifted column moves the result by percents"""
    nu = np.asarray(nu, float)
    i = np.arange(len(nu))
    f = 8.0 * np.sin(0.7 * i) + 0.01 * (i % 17)
    g = np.linspace(0.0, 1.0, nT) ** 2 * 20.0
    h = -np.sqrt(np.linspace(0.0, 1.0, nP)) * 13.0
    Z = f[:, None, None] + g[None, :, None] + h[None, None, :] + 0.3 * np.outer(np.arange(nT), np.arange(nP))[None] * np.cos(0.3 * i)[:, None, None]
    Z = Z - Z.min()
    return lo + 5.0 + Z * ((hi - lo - 10.0) / Z.max())


# ---- accelerated absorber ---------------------------------------------------------------------------------------------------------

def accel_sigma(L, Pknots, P):
    """exp(phi_i(ln P)), L[nk, nnu] = ln sigma on the knots: LinearInterpolator with NoBoundaries (absorbers.jl:195,203) -- the cell of
    ln P clamped to the end cells, which extrapolate.  Returns (sigma[nnu], factor) with factor = max(1, |x - xa| / (xb - xa))."""
    L = np.asarray(L, float)
    lnP = np.log(np.asarray(Pknots, float))
    xd = math.log(P)                                                    # the cell is chosen in double arithmetic, as any caller does
    c = int(_cells(lnP, np.array([xd]))[0])
    x, xa, xb = _ln(P, Pknots, lnP), mp.mpf(float(lnP[c])), mp.mpf(float(lnP[c + 1]))
    t = (x - xa) / (xb - xa)
    sig = np.array([float(mp.exp(t * (mp.mpf(float(L[c + 1, n])) - mp.mpf(float(L[c, n]))) + mp.mpf(float(L[c, n])))) for n in range(L.shape[1])])
    return sig, max(1.0, float(abs(t)), float(abs(1 - t)))


def accel_bound(L, factor):
    """8 U max|L| + 4 ulp, times the extrapolation factor"""
    return (8.0 * U * float(np.max(np.abs(L))) + 8.0 * U) * factor
