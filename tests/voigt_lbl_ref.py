"""Expected values of shape code 7, LBLRTM's line calculation at pressure-shifted centres (include/clearsky_hip.h, CS_SHAPE_VOIGT_LBL),
shared by tests/test_voigt_lbl.py (host) and tests/test_gpu_voigt_lbl.py (device).

    sigma_7(nu) = max(0, R(nu, T) sum_l S~_l [(f_l(nu - c_l) - f_l(D)) 1{|nu - c_l| <= D} + (f_l(nu + c_l) - f_l(D)) 1{nu + c_l <= D}])

with c_l = nul + s_l, s_l = delta_l P / P0, and S~_l, alpha_l, gamma_l from the unshifted nul.

`sigma_line` is ONE line at 40 digits: the code-6 branch of lineparam_ref.sigma_isolated restated with d = nu - (nul + s), the mirror
test and argument nu + nul + s, and S~, alpha, gamma from nul.  lineparam_ref.sigma_isolated(7, ...) is the same value with the terms
of its rounding bound beside it (test_voigt_lbl.py holds the two equal as floats); the per-line harnesses use that one.

`expected` is many lines through the oracle, by the identity the CS_SHAPE_PSHIFT tests use, extended for the mirror: line l's direct
term is the code-6 direct term on the grid nu - s_l, its mirror term the code-6 mirror term on the grid nu + s_l.  So for each distinct
shift s the lines sharing it give the oracle's Voigt of the S~-scaled table on nu - s minus their pedestals (ckdvvh_ref's window sums on
nu - s), plus their mirror terms minus theirs on nu + s; the sum over s is multiplied by R at the true nu.  The strict pre-filter of the
vector methods on the grid nu - s is nu_1 - D < nul + s < nu_N + D: the shifted centre's.  It returns (sigma, scale), the scale being R
times the sum of the magnitudes of every part -- the sum BEFORE the pedestal is subtracted (ckdvvh_ref.err).

`case_table` is the table of the device's exact-shift cases: every nul a multiple of 2^-6 (what the .par file's six decimals hold
exactly), every delta a multiple of 2^-5, so that with P a dyadic multiple of P0 and a dyadic grid nul + s, nu - s and nu + s + nul are
all exact in fp64 (`dyadic_premise`)."""
import mpmath as mp
import numpy as np

import ckdvvh_ref as X
import lineparam_ref as LP

KATM = LP.KATM
CUT = 25.0
_m = LP._m


def sigma_line(nu, line, T, P, Pp, cut, C=1.0, ends=None):
    """C x the 40-digit code-7 cross-section of ONE line (a lineparam_ref.line_of dict, with its delta) at the point nu, as (float value,
    float scale): scale = C R S~ (sum of profile values and pedestals present).  ends = (nu_1, nu_N): the vector methods' strict pre-filter
    on the shifted centre."""
    nul, v, D = _m(line["nu"]), _m(nu), _m(cut)
    c = nul + _m(line["delta"]) * _m(P) / _m(KATM)
    S, _, al, ga = LP.line_params(line, T, P, Pp, True)   # S / R(nul, T), alpha, gamma: from the unshifted nul
    if ends is not None and not (_m(ends[0]) - D < c < _m(ends[1]) + D):
        return 0.0, 0.0
    plus = minus = mp.mpf(0)
    if abs(v - c) <= D:
        plus += LP.fvoigt(v - c, al, ga)
        minus += LP.fvoigt(D, al, ga)
    if v + c <= D:
        plus += LP.fvoigt(v + c, al, ga)
        minus += LP.fvoigt(D, al, ga)
    r = v * mp.tanh(mp.mpf(LP.C2) * v / (2 * _m(T))) * _m(C)
    return float(max(S * (plus - minus) * r, mp.mpf(0))), float(S * (plus + minus) * r)


class _Tab:
    pass


def subset(sl, m):
    o = _Tab()
    for n in ("nu", "S", "gamma_a", "gamma_s", "Epp", "na", "mu", "I"):
        setattr(o, n, np.ascontiguousarray(getattr(sl, n)[m]))
    o.ncheb, o.cheb = sl.ncheb, sl.cheb
    return o


def expected(cs, O, sl, da, nu, T, P, Pp, cut=CUT, strict=True):
    """(sigma_7, scale) at the points nu for one state, the shifts da [cm^-1/atm] line for line"""
    nu = np.asarray(nu, float)
    s_l = np.asarray(da, float) * P / KATM
    ds = float(np.max(np.abs(s_l))) if len(s_l) else 0.0
    near = (sl.nu > nu[0] - cut - ds - 1.0) & (sl.nu < nu[-1] + cut + ds + 1.0)   # (the others add nothing on either grid)
    near |= sl.nu <= cut + ds + 1.0                                                # (the mirror lines)
    val, mag = np.zeros(len(nu)), np.zeros(len(nu))
    for s in np.unique(s_l[near]):
        sub = subset(sl, near & (s_l == s))
        xd, xm = nu - s, nu + s
        keep = X.included(sub, xd, cut, strict)
        j = np.nonzero(keep)[0]
        v = O.shape_bang("voigt", xd, X.tilde(cs, sub, T), T, P, Pp, cut, strict_ends=strict)
        p = np.zeros(len(sub.nu))
        if len(j):
            p[j] = X.line_terms(cs, O, sub, np.full(len(j), cut), T, P, Pp, j)
        ps = X.window_sum(sub.nu, p, xd, cut, keep)
        val += v - ps
        mag += v + ps
        for l in j:   # the mirror resonances at -(nul + s)
            m = ~(xm + sub.nu[l] > cut)
            if m.any():
                f = X.line_terms(cs, O, sub, xm[m] + sub.nu[l], T, P, Pp, np.full(int(m.sum()), l))
                val[m] += f - p[l]
                mag[m] += f + p[l]
    r = X.R(cs, nu, T)
    return np.maximum(r * val, 0.0), r * mag


def dyadic_premise(nul, nu, da, Ps):
    """nul + s, nu - s, nu + s and nu + (nul + s) are exact in fp64 (compared with extended precision)"""
    L = np.longdouble
    assert np.finfo(L).nmant > 60, "needs an extended long double"
    for P in Ps:
        s = da * P / KATM
        assert np.all(s == da * (P / KATM))
        c = nul + s
        assert np.all(L(nul) + L(s) == L(c))
        for sv in np.unique(s):
            assert np.all(L(nu) - L(sv) == L(nu - sv)) and np.all(L(nu) + L(sv) == L(nu + sv))
        assert np.all(L(nu)[:, None] + L(c)[None, :] == L(nu[:, None] + c[None, :]))
        assert np.all(L(nu)[:, None] - L(c)[None, :] == L(nu[:, None] - c[None, :]))


# ---- the tables and states of the device cases ------------------------------------------------------------------------------------

GRID = np.linspace(0.5, 64.5, 257)           # two 256-point tiles, the second ragged (one point); nu_1 below every cut-off used
EDGE_GRID = GRID[120:]                       # the edge cases' grid: from 30.5, so nu_1 - D lies among the lines for D = 1, 5 and 25
DELTAS = np.arange(-6, 5) / 32.0             # multiples of 2^-5 in [-0.1875, 0.125]
# nine states: one full octet of CS_PED_KC plus a tail; P a dyadic multiple of P0 including 0 and 2 P0
STATES = [(200.0, 0.0, 0.0), (215.0, 0.125, 0.01), (230.0, 0.25, 0.02), (245.0, 0.5, 0.0), (260.0, 1.0, 0.01), (275.0, 2.0, 0.005),
          (290.0, 0.75, 0.03), (305.0, 1.5, 0.0), (320.0, 2.0, 0.02)]   # (T, P / P0, Pp / P)


def states():
    T = [t for t, _, _ in STATES]
    P = [f * KATM for _, f, _ in STATES]
    Pp = [q * f * KATM for _, f, q in STATES]
    return T, P, Pp


def case_table(seed=11, L=220):
    """About L water-like lines on (0, 95) cm^-1 at multiples of 2^-6, ascending, delta drawn from DELTAS with the sign alternating along
    runs of neighbours; a few placed within the largest shift of every limit the grids GRID, EDGE_GRID and the cut-offs 1, 5 and 25 set (nu_1 - D,
    nu_N + D, D - nu_i, nu_i +- D), on both sides, with shifts of both signs.  Returns a dict of arrays for write_par."""
    rng = np.random.default_rng(seed)
    q = np.unique(rng.integers(1, 95 * 64, L))
    edge = []
    for D in (1.0, 5.0, 25.0):
        for lim in (GRID[0] - D, EDGE_GRID[0] - D, GRID[-1] + D, D - GRID[0], D - GRID[3], GRID[100] + D, GRID[100] - D, GRID[200] - D, GRID[31] + D):
            for off in (-0.125, -0.0625, -0.015625, 0.0, 0.015625, 0.0625, 0.125):
                if 0.015625 <= lim + off < 95.0:
                    edge.append(int(round((lim + off) * 64)))
    q = np.unique(np.concatenate([q, edge]))
    nul = q / 64.0
    n = len(nul)
    da = rng.choice(DELTAS, n)
    alt = rng.random(n) < 0.5   # runs of neighbours with alternating signs: shifted order reverses at pressure
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    da = np.where(alt, np.clip(np.abs(da) * sign, DELTAS[0], DELTAS[-1]), da)
    da = np.round(da * 32.0) / 32.0
    return dict(nu=nul, S=10.0 ** rng.uniform(-24, -19, n), gamma_a=np.round(rng.uniform(0.05, 0.10, n), 4), gamma_s=np.round(rng.uniform(0.2, 0.5, n), 3),
                Epp=np.round(rng.uniform(0, 2000, n), 4), na=np.round(rng.uniform(0.6, 0.8, n), 2), delta_a=da)


def membership(nul, da, nu, P, cut):
    """(direct, mirror) masks [point, line] by the shifted centre, and the same by the table position"""
    c = nul + da * P / KATM
    d = ~(np.abs(nu[:, None] - c[None, :]) > cut)
    m = ~(nu[:, None] + c[None, :] > cut)
    d0 = ~(np.abs(nu[:, None] - nul[None, :]) > cut)
    m0 = ~(nu[:, None] + nul[None, :] > cut)
    return d, m, d0, m0
