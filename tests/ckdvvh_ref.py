"""Expected values of shape code 6, the pedestal-removed Van Vleck-Huber Voigt (include/clearsky_hip.h, CS_SHAPE_VOIGT_CKD_VVH), shared
by tests/test_voigt_ckdvvh.py (host), tests/test_gpu_voigt_ckdvvh.py and tests/test_gpu_state_chunks.py (device).  The flags of `expected`
give its two halves at any cut-off: ped without vvh is code 4 (pedestal-removed Voigt), vvh without ped is code 5 (Van Vleck-Huber).

    sigma_6(nu) = max(0, R(nu, T) sum_l S~_l [(f_l(nu - nul) - f_l(cut)) 1{|nu - nul| <= cut} + (f_l(nu + nul) - f_l(cut)) 1{nu + nul <= cut}])

with R(x, T) = x tanh(c2 x / 2T) and S~_l = S_l / R(nul, T).  `expected` takes the direct Voigt part from the oracle's Voigt of the table
whose S is scaled by S~/S, and the per-line pedestals and mirror terms from `line_terms`, a vectorised restatement of S~_l f_l that
test_voigt_ckdvvh.py checks against one-line oracle slices and against 40-digit arithmetic.  It also returns the scale the device's
rounding is measured against: R times the sum of the magnitudes of every part (the pedestal difference cancels near each cut-off).
Without vvh there is no R, no S~ scaling and no mirror term; without ped no pedestal and no clamp."""
import math

import numpy as np

CUT = 25.0


def c2(cs):
    C_ = cs.constants
    return 100.0 * C_.h * C_.c / C_.k


def R(cs, x, T):
    """R(x, T) = x tanh(c2 x / 2T)"""
    return np.asarray(x, float) * np.tanh(c2(cs) * np.asarray(x, float) / (2.0 * T))


class _Tab:
    pass


def tilde(cs, sl, T, a=0, b=None, scale=True):
    """the lines [a, b) of sl with S scaled so that the oracle's S_l(T) becomes S_l(T) / R(nul, T) (scale=False: the plain slice)"""
    b = len(sl.nu) if b is None else b
    o = _Tab()
    for n in ("nu", "S", "gamma_a", "gamma_s", "Epp", "na", "mu", "I"):
        setattr(o, n, np.ascontiguousarray(getattr(sl, n)[a:b]))
    o.ncheb, o.cheb = sl.ncheb, sl.cheb
    if not scale:
        return o
    k2 = c2(cs)
    f = []
    for nl in o.nu:
        e = math.exp(-k2 * nl / T)
        f.append((1.0 + e) / (nl * (1.0 - e)))
    o.S = o.S * np.array(f)
    return o


def line_params(cs, O, sl, T, P, Pp, lines, vvh=True):
    """A_l = S~_l sqrt(ln 2 / pi) / alpha_l, d_l = sqrt(ln 2) / alpha_l and y_l = gamma_l d_l of the given lines, so that
    S~_l f_l(x) = A_l Re w(x d_l, y_l): S_l(T), alpha_l, gamma_l written out as the Voigt shape takes them (vvh=False: S_l, not S~_l)"""
    C_ = cs.constants
    j = np.asarray(lines, int)
    nul, E, I = sl.nu[j], sl.Epp[j], sl.I[j]
    k2 = c2(cs)
    qr = np.array([O.chebyQrefQ(T, sl.cheb[i][: sl.ncheb[i]]) if sl.ncheb[i] > 0 else np.nan for i in range(len(sl.ncheb))])
    # exp(-c2 nul / T) through the C library's exp (math.exp), as the oracle takes it: near nul = 0, 1 - exp(.) turns a one-ulp
    # difference of exp into eps / (c2 nul / T) ~ 3e-10 at the line at 8.4e-5 cm^-1
    xp = np.vectorize(math.exp, otypes=[float])
    d0 = np.exp(-k2 * E / C_.Tref) * (1.0 - xp(-k2 * nul / C_.Tref))
    e = xp(-k2 * nul / T)
    # S_l(T) as scaleintensity forms it, times (1 + e) / (nul (1 - e)) as tilde() scales it
    St = sl.S[j] * qr[I - 1] * (np.exp(-k2 * E / T) * (1.0 - e)) / d0
    if vvh:
        St = St * ((1.0 + e) / (nul * (1.0 - e)))
    alpha = (nul / C_.c) * np.sqrt(2.0 * C_.R * T / sl.mu[j])
    gamma = (C_.Tref / T) ** sl.na[j] * (sl.gamma_a[j] * (P - Pp) + sl.gamma_s[j] * Pp) / C_.atm
    d = np.sqrt(np.log(2.0)) / alpha
    return St * np.sqrt(np.log(2.0) / np.pi) / alpha, d, gamma * d


def line_terms(cs, O, sl, x, T, P, Pp, lines, vvh=True):
    """S~_l f_l(x_l) of each line at its own offset x_l (an array as long as lines); vvh=False: S_l f_l(x_l)"""
    A, d, y = line_params(cs, O, sl, T, P, Pp, lines, vvh)
    return A * O.faddeeva(np.asarray(x, float) * d, y)


def included(sl, nu, cut, strict):
    """the lines the shape includes: the vector methods' strict end-point pre-filter, or every line"""
    return (sl.nu > nu[0] - cut) & (sl.nu < nu[-1] + cut) if strict else np.ones(len(sl.nu), bool)


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


def window_sum(nul, p, x, cut, keep):
    """sum of p over each point's window among the included lines (contiguous), in extended precision"""
    g0 = int(np.argmax(keep)) if keep.any() else 0
    g1 = g0 + int(keep.sum())
    j0, j1 = windows(nul[g0:g1], x, cut)
    c = np.concatenate([[0.0], np.cumsum(p[g0:g1].astype(np.longdouble))])
    return (c[j1] - c[j0]).astype(float)


def expected(cs, O, sl, nu, T, P, Pp, cut=CUT, strict=True, ped=True, vvh=True):
    """(sigma, scale) at the points nu for one state: code 6 by default, code 4 with vvh=False, code 5 with ped=False"""
    nu = np.asarray(nu, float)
    keep = included(sl, nu, cut, strict)
    j = np.nonzero(keep)[0]
    v = O.shape_bang("voigt", nu, tilde(cs, sl, T) if vvh else sl, T, P, Pp, cut, strict_ends=strict)
    p = np.zeros(len(sl.nu))
    if ped and len(j):
        p[j] = line_terms(cs, O, sl, np.full(len(j), cut), T, P, Pp, j, vvh)
    ps = window_sum(sl.nu, p, nu, cut, keep) if ped else 0.0
    s, mag = v - ps, v + ps
    if vvh:
        for l in j[sl.nu[j] <= cut - nu[0] + 1e-9]:   # the mirror resonances
            m = ~(nu + sl.nu[l] > cut)
            if m.any():
                f = line_terms(cs, O, sl, nu[m] + sl.nu[l], T, P, Pp, np.full(int(m.sum()), l))
                s[m] += f - p[l]
                mag[m] += f + p[l]
        r = R(cs, nu, T)
        s, mag = r * s, r * mag
    return (np.maximum(s, 0.0) if ped else s), mag


def err(s, ref):
    """max |s - sigma| / scale; 0 where the scale is (no line reaches the point, or nu = 0) only if s is exactly 0 there"""
    val, scale = ref
    s = np.asarray(s, float)
    z = scale == 0.0
    if np.any(s[z] != 0.0):
        return np.inf
    return float(np.max(np.abs(s[~z] - val[~z]) / scale[~z])) if (~z).any() else 0.0
