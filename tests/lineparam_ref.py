"""40-digit reference of the per-(state, line) parameter stage -- what prep_body (csrc/cs_kernels.h) forms for every line kernel -- and the
probe sets that reach it one line at a time, shared by tests/test_lineparam_ref.py (host: the oracle, closed forms, the measurement of
c0) and tests/test_gpu_lineparams.py (device).  Everything is computed in mpmath from the double inputs exactly; no oracle, no GPU.

Restated from the reference's absorption/line_shapes.jl:
  qrefq            chebyQrefQ (:27-48): 1 / sum a_k T_k(tau), tau = 2 (T - TMIN) / (TMAX - TMIN) - 1, and its condition sum |a_k T_k| / |y|
  intensity        scaleintensity (:107-123): S Qref/Q(T) exp(a/T) (1 - exp(b/T)) / [exp(a/Tref) (1 - exp(b/Tref))], a = -c2 Epp, b = -c2 nul
  alpha_doppler    alphadoppler (:144): (nul / c) sqrt(2 R T / mu)
  gamma_lorentz    gammalorentz (:255-257): (Tref / T)^na (gamma_a (P - Pp) + gamma_s Pp) / atm
  florentz, fdoppler, fvoigt   (:273, :160, :366-378) with w(z) = exp(-z^2) erfc(-i z)
  chi (code 3)     XPHCO2 (:467-481): 1 below 3 cm^-1, exp(-B1 (d - 3)) on [3, 30), exp(-27 B1 - B2 (d - 30)) on [30, 120), exp(-27 B1 - 90 B2 -
                   B3 (d - 120)) beyond, B1 = 0.0888 - 0.16 exp(-0.0041 T), B2 = 0.0526 exp(-0.00152 T), B3 = 0.0232; PHCO2 (:496-499) is
                   fvoigt(d, alpha, chi gamma).  B1 < 0 below T = 143.6 K: chi > 1 there in region 1 and well into region 2
and from include/clearsky_hip.h: code 4's pedestal f(cut), code 5's R(x, T) = x tanh(c2 x / 2T), S~ = S / R(nul, T) and mirror term
f(nu + nul) where nu + nul <= cut, code 6 (both), the CS_SHAPE_PSHIFT centre nul + delta P / P0 (S, alpha, gamma from the unshifted nul),
and code 7: code 6 with both cut-off tests and the mirror argument measured from that centre.
c2 = 100 h c / k is the double the sources form (line_shapes.jl:5), sqrt(ln 2), sqrt(pi) are exact.

sigma_isolated(shape, nu, line, T, P, Pp, cut, C) is C x the cross-section of ONE line at one point with the pieces the bound needs;
lineparam_bound(info, c0) is the first-order rounding model (its docstring names every term).

The constant c0 -- how it is measured.  test_lineparam_ref.py::test_measure_c0 takes, over every probe the device tests use, the worst
of (oracle error) / 2^-53 - (the model's terms without c0): the smallest constant with which the model holds for the oracle.  It prints
that figure per shape code, with the worst ratio (oracle error) / (2^-53 x terms) beside it.

Recorded figures (this project's oracle, built as build() builds it, glibc's libm):
  Lorentz (code 1)              4.99
  Doppler (code 2)              4.32
  shifted codes (16, 17, 18)    0.95 and less
  code 7                        0 beyond the Faddeeva allowance and its centre term; the oracle composite the device's code-7 tests
                                use (voigt_lbl_ref.expected on one-line tables) reaches 0.68 of the bound, at a probe the centre term leads
  Voigt codes (0, 4, 5, 6)      0 beyond the Faddeeva allowance.  That allowance is 1800 x 2^-53 and dominates their bound, so these
                                codes see errors of this stage from about 2e-13 on only.
  C0_ORACLE = 5.0               the worst of these, 4.99, rounded up to two digits

The rule.  test_measure_c0 asserts measured <= C0_ORACLE with no margin beyond that rounding, knowingly: the device's bound is derived
from the recorded value, so the recorded value must not drift from what the oracle does.  A failure of that assertion alone -- after a
change of compiler or libm, say, that moves one rounding of the oracle -- therefore means "measure again and record the new figure
here", not a fault in the library; the device tests then run with the new C0_GPU.  A device failure is never answered by raising c0.

The device is held to C0_GPU = GPU_FACTOR x C0_ORACLE = 20.  Its exp is good to 2 ulp against libm's < 1, its divisions are v_rcp +
Newton steps, its sums are FMA-contracted, and the host folds the Tref factor into sref (one more rounding and a division).  So each of
the oracle's roundings may count up to four times.

Values below 1e-290 (UNDERFLOW) are not compared relatively: the result must be finite, >= 0 and < 1e-289; at most 10 % of the probes
of one test may be of that class (`split`).
"""
import math

import mpmath as mp
import numpy as np

from clearsky_jl_amd import constants as C_
from clearsky_jl_amd import hitran as H

mp.mp.dps = 40
U = 2.0 ** -53
C2 = 100.0 * C_.h * C_.c / C_.k          # the double of line_shapes.jl:5
FADDEEVA = 2e-13                         # what test_faddeeva_device asserts of the device's Re w against 40-digit goldens
UNDERFLOW = 1e-290
C0_ORACLE = 5.0
GPU_FACTOR = 4.0
C0_GPU = GPU_FACTOR * C0_ORACLE
PSHIFT = 16
VOIGT_CODES = (0, 4, 5, 6)
LBL = 7                                  # CS_SHAPE_VOIGT_LBL: code 6 at the shifted centres, without the flag


def shifts(code):
    """the code places its lines at nul + delta P / P0: CS_SHAPE_PSHIFT on codes 0-2, or code 7"""
    return bool(code & PSHIFT) or code == LBL

_m = lambda x: mp.mpf(float(x))
_SQLN2 = mp.sqrt(mp.log(2))
_SQPI = mp.sqrt(mp.pi)


def line_of(sl, j, delta=None):
    """line j of a SpectralLines-like table as a dict of doubles (cheb: the fit's coefficients, empty without a fit)"""
    i = int(sl.I[j]) - 1
    d = sl.delta_a[j] if (delta is None and getattr(sl, "delta_a", None) is not None) else (delta or 0.0)
    return dict(nu=float(sl.nu[j]), S=float(sl.S[j]), gamma_a=float(sl.gamma_a[j]), gamma_s=float(sl.gamma_s[j]), Epp=float(sl.Epp[j]),
                na=float(sl.na[j]), mu=float(sl.mu[j]), cheb=np.array(sl.cheb[i, : int(sl.ncheb[i])], float), delta=float(d))


def qrefq(T, a):
    """(Qref/Q(T), condition number sum |a_k T_k(tau)| / |sum a_k T_k(tau)|) -- line_shapes.jl:27-48"""
    tau = 2 * (_m(T) - _m(H.TMIN)) / (_m(H.TMAX) - _m(H.TMIN)) - 1
    c1, c2 = mp.mpf(1), tau
    y = _m(a[0]) + _m(a[1]) * c2
    s = abs(_m(a[0])) + abs(_m(a[1]) * c2)
    for k in range(2, len(a)):
        c3 = 2 * tau * c2 - c1
        y += _m(a[k]) * c3
        s += abs(_m(a[k]) * c3)
        c1, c2 = c2, c3
    return 1 / y, float(s / abs(y))


def intensity(line, T, vvh=False):
    """(S(T), Q condition) of scaleintensity (:107-123); vvh: S(T) / R(nul, T), R(x, T) = x tanh(c2 x / 2T) (clearsky_hip.h, code 5)"""
    a, b = -mp.mpf(C2) * _m(line["Epp"]), -mp.mpf(C2) * _m(line["nu"])
    T_, Tr = _m(T), _m(C_.Tref)
    q, cond = qrefq(T, line["cheb"])
    S = _m(line["S"]) * q * (mp.exp(a / T_) * (1 - mp.exp(b / T_))) / (mp.exp(a / Tr) * (1 - mp.exp(b / Tr)))
    if vvh:
        S = S / (_m(line["nu"]) * mp.tanh(-b / (2 * T_)))
    return S, cond


def alpha_doppler(line, T):
    return (_m(line["nu"]) / _m(C_.c)) * mp.sqrt(2 * _m(C_.R) * _m(T) / _m(line["mu"]))


def gamma_lorentz(line, T, P, Pp):
    return (_m(C_.Tref) / _m(T)) ** _m(line["na"]) * (_m(line["gamma_a"]) * (_m(P) - _m(Pp)) + _m(line["gamma_s"]) * _m(Pp)) / _m(C_.atm)


def florentz(d, g):
    return g / (mp.pi * (d * d + g * g))


def fdoppler(d, a):
    return mp.exp(-(d * d) / (a * a)) / (a * _SQPI)


def fvoigt(d, a, g, slope=False):
    """fvoigt (:366-378); slope: also d ln f / d d = -2 Re(z w) / Re w x sqrt(ln 2) / alpha, from w' = -2 z w + 2i / sqrt(pi)"""
    dd = _SQLN2 / a
    z = mp.mpc(d * dd, g * dd)
    w = mp.exp(-z * z) * mp.erfc(-1j * z)
    f = (_SQLN2 / _SQPI) / a * w.real
    if not slope:
        return f
    return f, (-2 * (z * w).real / w.real * dd if w.real != 0 else mp.mpf(0))


def widths(line, T, P, Pp):
    """(alpha, gamma) as doubles: what the probe offsets are multiples of"""
    return float(alpha_doppler(line, T)), float(gamma_lorentz(line, T, P, Pp))

PH_D = (3.0, 30.0, 120.0)                # the region boundaries of XPHCO2 (:469, :473, :477)


def ph_coefs(T):
    """(B1, B2, B3) of XPHCO2 (:472, :476, :480) at 40 digits from the doubles the source writes"""
    T_ = _m(T)
    return _m(0.0888) - _m(0.16) * mp.exp(-_m(0.0041) * T_), _m(0.0526) * mp.exp(-_m(0.00152) * T_), _m(0.0232)


def ph_coef_abs(T):
    """per coefficient B_q: what U multiplies in the absolute error of a double evaluation of it, plus 3 |B_q| for the roundings of a
    product B_q x m (the factor m, the product, the sum it joins) -- B1: the final subtraction rounds to U |B1| <= U 0.0888, the
    subtrahend 0.16 e^(-0.0041 T) carries its argument's rounding (0.0041 T), the exponential's (1, 2 on the device: inside the count of 3) and the
    product's; B2 likewise; B3 is the source's own double"""
    B1, B2, B3 = (float(b) for b in ph_coefs(T))
    e1 = math.exp(-0.0041 * T)
    return (0.0888 + 0.16 * e1 * (3.0 + 0.0041 * T) + 3.0 * abs(B1), B2 * (3.0 + 0.00152 * T) + 3.0 * B2, 3.0 * B3)


def chi_phco2(d, T, side=0):
    """(chi, region 0..3, (m1, m2, m3)) of XPHCO2 at the distance d >= 0: chi = exp(-(B1 m1 + B2 m2 + B3 m3)); side = -1 / +1 evaluates
    the formula of the region below / above where d sits exactly on a boundary (the continuity test), 0 the source's own choice"""
    B = ph_coefs(T)
    r = sum(1 for D in PH_D if d >= D)
    if side < 0 and d in [_m(D) for D in PH_D]:
        r -= 1
    m = (mp.mpf(0),) * 3 if r == 0 else (d - 3, 0, 0) if r == 1 else (mp.mpf(27), d - 30, 0) if r == 2 else (mp.mpf(27), mp.mpf(90), d - 120)
    chi = mp.mpf(1) if r == 0 else mp.exp(-sum(b * x for b, x in zip(B, m)))
    return chi, r, tuple(float(x) for x in m)


_PARAMS = {}


def line_params(line, T, P, Pp, vvh=False):
    """(S(T), Q condition, alpha, gamma) at 40 digits, kept per (line, state): every probe of a pair shares them"""
    key = (line["nu"], line["S"], line["gamma_a"], line["gamma_s"], line["Epp"], line["na"], line["mu"], line["cheb"].tobytes(), T, P, Pp, vvh)
    if key not in _PARAMS:
        if len(_PARAMS) > 4096:
            _PARAMS.clear()
        _PARAMS[key] = intensity(line, T, vvh) + (alpha_doppler(line, T), gamma_lorentz(line, T, P, Pp))
    return _PARAMS[key]


def sigma_isolated(shape, nu, line, T, P, Pp, cut, C=1.0):
    """C x the 40-digit cross-section of ONE line at the point nu under shape code `shape` (0, 1, 2, 3, 4, 5, 6, 7; | 16 = CS_SHAPE_PSHIFT
    on 0-2), as (float value, mpf value, info); info holds S, alpha, gamma (doubles) and the terms of lineparam_bound.  Code 7 is code 6
    with both cut-off tests and the mirror argument measured from c = nul + delta P / P0, S~, alpha and gamma from the unshifted nul
    (voigt_lbl_ref.sigma_line is the same value).  Code 3 (PHCO2):
    the profile is fvoigt(d, alpha, chi gamma), the cut-off inclusive as for code 0; info gains chi, region (0: |d| < 3, 1 .. 3), chi_m
    (the multipliers m_q of B_q in chi's exponent), chi_abs (ph_coef_abs) and chi_rnd, the rounding term of chi as ONE exponential."""
    base, psh = shape & ~PSHIFT, bool(shape & PSHIFT)
    assert base in (0, 1, 2, 3, 4, 5, 6, 7) and not (psh and base > 2)
    lbl = base == 7                                       # code 6 at the shifted centre: it takes the shifts without the flag
    vvh, ped = base in (5, 6, 7), base in (4, 6, 7)
    nul, v, D = _m(line["nu"]), _m(nu), _m(cut)
    s = _m(line["delta"]) * _m(P) / _m(C_.atm) if psh or lbl else mp.mpf(0)
    c = nul + s
    d = v - c
    S, qcond, al, ga = line_params(line, T, P, Pp, vvh)
    x_T, x_r = C2 * line["nu"] / T, C2 * line["nu"] / C_.Tref
    pl = lambda x: float((1 + x) / mp.expm1(_m(x)))
    info = dict(shape=shape, S=float(S), alpha=float(al), gamma=float(ga), qcond=qcond, a_T=abs(C2 * line["Epp"] / T),
                a_ref=abs(C2 * line["Epp"] / C_.Tref), planck_T=0.0 if vvh else pl(x_T), planck_ref=pl(x_r),
                pow=abs(line["na"] * math.log(C_.Tref / T)), doppler=0.0, alpha7=0.0, centre=0.0, chi_rnd=0.0,
                voigt=base in VOIGT_CODES or base in (3, 7), rel=1.0)
    slope = mp.mpf(0)
    if base == 1:
        f = lambda t: florentz(t, ga)
        slope = -2 * d / (d * d + ga * ga) if psh else slope
    elif base == 2:
        f = lambda t: fdoppler(t, al)
        slope = -2 * d / (al * al)
        info["doppler"] = float(2 * (d / al) ** 2)
        info["alpha7"] = float(7 * (d / al) ** 2)
    elif base == 3:
        chi, region, m = chi_phco2(abs(d), T)
        f = lambda t: fvoigt(t, al, chi * ga)
        cabs = ph_coef_abs(T)
        info.update(chi=float(chi), region=region, chi_m=m, chi_abs=cabs, chi_rnd=chi_rounding(m, cabs, 1) if region else 0.0)
    else:
        f = lambda t: fvoigt(t, al, ga)
        if psh:
            slope = fvoigt(d, al, ga, slope=True)[1]
    if psh and s != 0:   # the device rounds delta P, / P0 and the sum: |dc| <= U (|c| + 2 |s|), times the profile's |d ln f / d nu|
        info["centre"] = float(abs(slope) * (abs(c) + 2 * abs(s)))
    plus = minus = mp.mpf(0)
    moved = mp.mpf(0)    # code 7: sum over the terms present of |df / dc| x what U multiplies in the error of the term's argument
    exact = lambda t: _m(float(t)) == t
    c_exact = exact(_m(line["delta"]) * _m(P)) and exact(s) and exact(c)      # (every operation behind the device's centre is exact)
    for x, inside in ((d, abs(d) <= D), (v + (c if lbl else nul), vvh and v + (c if lbl else nul) <= D)):
        if not inside:
            continue
        if lbl:
            fx, sl = fvoigt(x, al, ga, slope=True)
            # the centre's own rounding (none without a shift), and the rounding of nu -+ c where that is no double (lineparam_bound)
            moved += abs(sl) * fx * ((abs(c) + 2 * abs(s) if s != 0 else 0) + (0 if c_exact and exact(x) else abs(x)))
        else:
            fx = f(x)
        plus += fx
        minus += f(D) if ped else 0
    if lbl and plus > 0:
        info["centre"] = float(moved / plus)
    val = S * (plus - minus)
    if vvh:
        val *= v * mp.tanh(mp.mpf(C2) * v / (2 * _m(T)))
    if ped:
        val = max(val, mp.mpf(0))
        info["rel"] = float((plus - minus) / plus) if plus > 0 else 1.0
        # the profile part alone, C S R x the sum of the profile values: what rel x the value tends to where the pedestal takes it all off
        info["mag"] = float(S * plus * (v * mp.tanh(mp.mpf(C2) * v / (2 * _m(T))) if vvh else 1) * _m(C))
    val *= _m(C)
    return float(val), val, info


def chi_rounding(mult, cabs, nexp):
    """code 3: what U multiplies in the relative rounding error of chi = a product of `nexp` exponentials whose arguments are sums of
    B_q x (multipliers adding up to mult[q]): sum_q mult[q] x ph_coef_abs[q] -- the arguments' absolute errors, which are chi's relative
    ones -- plus 2 per exponential (the device's exp: 2 ulp, module docstring).  The profile is at most linear in chi beyond 3 cm^-1
    (|d ln K(x, chi y) / d ln chi| = |1 - 2 (chi y)^2 / s| <= 1 for the Lorentz-like wing, s >= 1e4), so the term enters with factor 1."""
    return sum(a * b for a, b in zip(mult, cabs)) + 2.0 * nexp


def model_terms(info):
    """the bracket of lineparam_bound without c0"""
    return (info["a_T"] + info["a_ref"] + info["planck_T"] + info["planck_ref"] + info["qcond"] + info["pow"] + info["doppler"]
            + info["alpha7"] + info["centre"] + info.get("chi_rnd", 0.0))


def lineparam_bound(info, c0):
    """Relative error a double evaluation of one line's cross-section may have against sigma_isolated -- a first-order rounding model:

        [ U (c0 + |a/T| + |a/Tref| + p(c2 nul/T) + p(c2 nul/Tref) + Qcond + |na ln(Tref/T)| + (2 + 7) (dnu/alpha)^2 + chi + centre) + F ] / rel

      |a/T|, |a/Tref|     exp(a/T), a = -c2 Epp: a relative rounding of its argument moves it by |a/T| of itself; likewise at Tref
      p(x) = (1+x)/(e^x-1) 1 - exp(-x) at x = c2 nul / T: the argument's rounding (x e^-x / (1 - e^-x)) and the rounding of exp(-x) before the
                          subtraction (e^-x / (1 - e^-x)); codes 5 and 6 form (1 + exp(-x)) / nul instead (clearsky_hip.h: the factor cancels
                          exactly) and have no such term at T -- only the one at Tref, which every code has
      Qcond               sum |a_k T_k(tau)| / |sum a_k T_k(tau)| of the Chebyshev sum behind Qref/Q
      |na ln(Tref/T)|     (Tref/T)^na = exp(na ln(Tref/T)): the rounding of the exponent
      2 (dnu/alpha)^2     Doppler only: exp(-(dnu/alpha)^2) moves by twice its exponent per relative rounding of alpha
      7 (dnu/alpha)^2     Doppler only: the other roundings that reach that exponent e = dnu^2 / alpha^2.  alpha = (nul / c) sqrt(2 R T / mu) carries
                          3 U (the quotient nul / c; the product and the quotient under the root, halved by it; the root; the product), so
                          alpha^2 carries 2 x 3 + 1 = 7, dnu^2 one and the quotient one: 9 U e in all, of which the term above names 2
      chi                 code 3 beyond 3 cm^-1: chi_rounding -- the scalar form (one exponential) here; tests/phco2_line_ref.py replaces it by
                          the factorised form's (two exponentials about the grid's centre) where the fast path serves the probe
      centre              CS_SHAPE_PSHIFT with a non-zero shift s = delta P / P0 only: the device rounds delta P, the division and the sum,
                          |dc| <= U (|c| + 2 |s|) on the centre c = nul + s, while nu - c is exact here; times |d ln f / d nu| of the profile at
                          the probe (2 |d| / (d^2 + gamma^2), 2 |d| / alpha^2, or the Voigt profile's own slope)
                          Code 7 has two profile terms that hang on the centre, the direct f(nu - c) and, where nu + c <= cut, the mirror
                          f(nu + c); the pedestals f(cut) do not.  The device forms c as above, so dc moves the bracket
                          f(nu - c) + f(nu + c) by at most U (|c| + 2 |s|) (|f'(nu - c)| + |f'(nu + c)|); relative to that bracket this is
                              centre = (|c| + 2 |s|) sum_i |d ln f / d x|(x_i) f(x_i) / sum_i f(x_i),   x_i = nu - c, nu + c (those present),
                          each term's slope weighted by its share of the sum.  The arguments themselves are rounded once more where
                          they are no doubles: x_i = fl(nu -+ c) carries U |x_i|, which the slope turns into U |x_i| |d ln f / d x|(x_i)
                          of its term.  That is added under the same weights unless delta P, its quotient by P0, c and x_i are all
                          exact in fp64 (dyadic shifts, pressures and probes), where the device's argument is the exact one; with s = 0
                          (delta = 0 or P = 0) c is nul itself and only this part can remain.  Division by rel, below, then refers
                          the sum to the bracket minus its pedestals, as for code 6      c0                  every rounding whose amplification is 1 (products, quotients, square root, the constants): measured, see the
                          module docstring
      F                   Voigt codes and code 3: 2e-13, the Faddeeva allowance
      rel                 codes 4, 6 and 7: (profile - pedestal) / profile at the probe, 1 otherwise.  Exactly on the cut-off the value
                          and rel are 0 and the relative bound is infinite; its absolute form stays: |error| <= [...] x info["mag"], the
                          profile part alone"""
    num = U * (c0 + model_terms(info)) + (FADDEEVA if info["voigt"] else 0.0)
    return num / info["rel"] if info["rel"] > 0.0 else math.inf      # (a probe exactly on the cut-off of a pedestal code: see info["mag"])


def split(vals):
    """(mask of the probes compared relatively, share of the underflow class)"""
    m = np.abs(np.asarray(vals, float)) >= UNDERFLOW
    return m, float(1.0 - np.mean(m)) if len(m) else 0.0


def check(got, want, bounds, zero, what=""):
    """got against the 40-digit doubles `want` within `bounds` (relative); underflow-class probes finite, >= 0, < 1e-289 and at most 10 %
    of all; probes whose 40-digit value is exactly 0 (`zero`: no term within the cut-off) exactly 0.  Returns the worst error / bound."""
    got, want, bounds = (np.asarray(t, float) for t in (got, want, bounds))
    zero = np.asarray(zero, bool)
    assert np.all(got[zero] == 0.0), what
    m, share = split(want[~zero])
    assert share <= 0.10, (what, share)
    g, w, b = got[~zero], want[~zero], bounds[~zero]
    assert np.all(np.isfinite(g[~m]) & (g[~m] >= 0.0) & (g[~m] < 1e-289)), what
    r = np.abs(g[m] - w[m]) / np.abs(w[m]) / b[m]
    worst = float(np.max(r)) if r.size else 0.0
    assert worst <= 1.0, (what, worst, int(np.argmax(r)))
    return worst


# ---- probe sets -------------------------------------------------------------------------------------------------------------------

KATM = C_.atm
K_SETS = (1, 7, 8, 9, 17)                      # CS_PREP_KC = 8 states per thread: both sides of one and of two chunks
T_EDGE = (25.0, 26.0, 100.0, 296.0, 999.0, 1000.0)
P_EDGE = ((1e-2, 0.0), (1e5, 5e4), (1e7, 1e7))
OFFSETS = (0.0, 0.5, -1.0, 3.0, -0.5, 1.0, -3.0)


def table(cs, M, iso, nu, S, ga, gs, Epp, na):
    n = len(nu)
    full = lambda x: np.full(n, x, float) if np.ndim(x) == 0 else np.asarray(x, float)
    return cs.SpectralLines(dict(M=np.full(n, M, np.int16), I=np.asarray(iso, np.int16), nu=full(nu), S=full(S), gamma_a=full(ga),
                                 gamma_s=full(gs), Epp=full(Epp), na=full(na)))


def states(K, seed, with_vacuum=False):
    """K states cycling through the edge temperatures (all six from K = 7 on) and pressures; with_vacuum: (0, 0) among the pressures"""
    Ps = P_EDGE + (((0.0, 0.0),) if with_vacuum else ())
    return [(T_EDGE[(k + seed) % 6], *Ps[(k // 2 + seed) % len(Ps)]) for k in range(K)]


def probes(lines, sts, base, cut, nside=3, far=False, centres=None):
    """The grid of a call and, per state, the probes compared there: for every line the centre and `nside` of the offsets of 1/2, 1 and 3
    widths (alternating sides) of that state, inside the cut-off and at nu > 0; far: also 0.9 cut on one side and 1.1 cut (beyond the
    cut-off) on the other.  The width is alpha (Doppler), gamma (Lorentz) or their sum (Voigt codes).  centres[k][l]: the state's own
    (shifted) centre.
    Returns (nu, [(k, index into nu, line index)])."""
    pts = []
    for k, (T, P, Pp) in enumerate(sts):
        for l, ln in enumerate(lines):
            al, ga = widths(ln, T, P, Pp)
            if base == 1 and ga == 0.0:      # (Lorentz of zero width -- P = 0, or Pp = P with gamma_self = 0: the reference itself is 0/0)
                continue
            w = al if base == 2 else ga if base == 1 else al + ga
            c = ln["nu"] if centres is None else centres[k][l]
            offs = [o * w for o in OFFSETS[(l + k) % 2 * 3: (l + k) % 2 * 3 + 1 + nside]]
            offs[0] = 0.0
            offs = [o for o in offs if abs(o) < 0.95 * cut]
            if far and ga > 0.0:   # (gamma = 0: the profile at 0.9 cut is a pure Gaussian tail hundreds of orders below the centre, which
                # the Faddeeva far-wing region -- not this stage -- returns as 0)
                sg = 1.0 if (l + k) % 2 else -1.0
                offs += [0.9 * cut * sg, -1.1 * cut * sg]
            pts += [(k, c + o, l) for o in offs if c + o > 0]
    nu = np.unique([p[1] for p in pts])
    return nu, [(k, int(np.searchsorted(nu, v)), l) for k, v, l in pts]


def lines_within(nul, v, cut):
    """how many table lines lie within the cut-off of the point v (the scalar methods' includedlines, :12-16)"""
    return int(np.sum(np.abs(np.asarray(nul) - v) <= cut))


# edge parameters: six line positions per table, the other parameters by a seeded choice
NU_EDGE = (0.05, 2.0, 50.0, 667.0, 3000.0, 15000.0)
EPP_EDGE = (-1.0, 0.0, 1e-3, 300.0, 3000.0, 2e4)
NA_EDGE = (-0.5, 0.0, 0.5, 1.2)
GS_EDGE = (0.0, 0.1)
S_EDGE = (1e-30, 1e-19)
CUT_EDGE = 0.9                                  # below half the smallest gap (0.05 -> 2): every probe sees one line, mirrors included
N_EDGE_TABLES = 20


def edge_tables(cs):
    """[(table, K, seed)]: CO2-like tables of one line per position of NU_EDGE; table t takes K_SETS[t % 5] states.  Every value of every
    parameter meets every temperature of T_EDGE in some state of its table (asserted pair by pair below).

    120 lines in 20 tables is a deliberate reduction from the few hundred lines first planned for this set: each line is evaluated in
    mpmath at up to 6 probes in each of up to 17 states under each of 6 shape codes, and that cost, not the device's, sets the tests' time.
    What the larger set was for -- every value of every parameter with every temperature -- is what the assertion holds at 120."""
    rng = np.random.default_rng(20240)
    out, seen = [], set()
    for t in range(N_EDGE_TABLES):
        n = len(NU_EDGE)
        E = [EPP_EDGE[(t + i) % 6] for i in range(n)]                       # a Latin square of positions and lower-state energies
        na = [NA_EDGE[(t // 2 + i + int(rng.integers(4))) % 4] for i in range(n)]
        gs = [GS_EDGE[(t + i // 2 + int(rng.integers(2))) % 2] for i in range(n)]
        S = [S_EDGE[(t // 3 + i + int(rng.integers(2))) % 2] for i in range(n)]
        iso = [1 + (t + i) % 12 for i in range(n)]
        K = K_SETS[t % 5]
        for T in {st[0] for st in states(K, t)}:
            seen |= {(n_, x, T) for n_, xs in (("nu", NU_EDGE), ("E", E), ("na", na), ("gs", gs), ("S", S)) for x in xs}
        out.append((table(cs, 2, iso, NU_EDGE, S, 0.07, gs, E, na), K, t))
    want = {(n_, x, T) for n_, xs in (("nu", NU_EDGE), ("E", EPP_EDGE), ("na", NA_EDGE), ("gs", GS_EDGE), ("S", S_EDGE)) for x in xs for T in T_EDGE}
    assert seen == want
    return out


# CS_SHAPE_PSHIFT: one table read from a .par file (the library takes the shifts from the file alone)
DELTA_EDGE = (0.0, 0.002, -0.01, 0.01, -0.005, 0.25)      # delta of both signs and 0; the last is dyadic (filter_case)
ISOCHAR = "1234567890AB"


def _fx(x, w, dec):
    """x in a fixed field of w characters (HITRAN drops the leading zero where the field needs it)"""
    r = f"{x:.{dec}f}"
    r = r.replace("0.", ".", 1) if len(r) > w else r
    assert len(r) <= w, (x, w)
    return r.rjust(w)


def shifted_table(cs, directory):
    """a CO2-like table of one line per position of NU_EDGE with the shifts DELTA_EDGE, written as a HITRAN 160-column file (par.jl:131-149
    layout) and read back: the values the fixed-width fields hold are the table's"""
    path = str(directory) + "/lineparam_shift.par"
    E, na, gs, S = (300.0, -1.0, 2e4, 0.0, 3000.0, 1e-3), (0.5, -0.5, 1.2, 0.0, 0.5, 1.2), (0.1, 0.0, 0.1, 0.0, 0.1, 0.1), (1e-19, 1e-30) * 3
    with open(path, "w") as f:
        for j, v in enumerate(NU_EDGE):
            r = (f"{2:2d}{ISOCHAR[(3 * j) % 12]}{v:12.6f}{S[j]:10.3E}{1.0:10.3E}{_fx(0.07, 5, 4)}{_fx(gs[j], 5, 3)}{E[j]:10.4f}"
                 f"{_fx(na[j], 4, 2)}{_fx(DELTA_EDGE[j], 8, 5)}")
            assert len(r) == 67, r
            f.write(r + " " * 93 + "\n")
    sl = cs.SpectralLines(path)
    assert np.array_equal(sl.delta_a, DELTA_EDGE) and np.array_equal(sl.nu, NU_EDGE)
    return sl


def shifted_centres(sl, sts):
    """centres[k][l] = nul + delta P / P0 in doubles, as a caller would place its probes"""
    return [[float(sl.nu[l] + sl.delta_a[l] * P / KATM) for l in range(len(sl.nu))] for _, P, _ in sts]


# the strict end-point filter of the vector methods is measured from the SHIFTED centre and differs from the inclusive cut-off only at
# equality: with cut = 1, the line at 15000 (delta = 0.25, dyadic) and a grid ending at 14999.5, the centre at P = 2 atm is 15000.5 =
# nu_N + cut exactly (every operation exact in fp64) -- the line leaves the filter in that state only: cs_shape_batch gives an exact 0 at
# every point there, the full value in the other states; cs_shape_points (no pre-filter) the full value at nu_N, |nu_N - c| = cut, too
FILTER_CUT = 1.0
FILTER_GRID = (14998.9, 14999.2, 14999.5)
FILTER_STATES = ((296.0, 2.0 * KATM, 1e3), (296.0, KATM, 1e3), (250.0, 0.5 * KATM, 0.0))


def expected(shape, sl, sts, nu, pr, cut, C=None, deltas=None, c0=C0_GPU, infos=None):
    """(want[len(pr)], bound[len(pr)], zero[len(pr)]) of the probes pr = [(k, i, l)] of a call; zero: the 40-digit value is exactly 0"""
    lines = [line_of(sl, l, None if deltas is None else deltas[l]) for l in range(len(sl.nu))]
    want, bnd, zero = np.zeros(len(pr)), np.zeros(len(pr)), np.zeros(len(pr), bool)
    for q, (k, i, l) in enumerate(pr):
        T, P, Pp = sts[k]
        want[q], v, info = sigma_isolated(shape, nu[i], lines[l], T, P, Pp, cut, 1.0 if C is None else C[k])
        bnd[q], zero[q] = lineparam_bound(info, c0), v == 0
        if infos is not None:
            infos.append(info)
    return want, bnd, zero


# every isotopologue: per molecule one line per isotopologue with a fit, at spread positions
CUT_ISO = 2.0
T_ISO = (25.0, 296.0, 1000.0, 137.31, 612.77)     # the ends of the fit (tau = -1, +1), Tref, two seeded values


def iso_table(cs, M):
    mpar = cs.MOLPARAM[M]
    iso = [i + 1 for i in range(len(mpar.I)) if mpar.hascheb[i]]
    n = len(iso)
    nu = 400.0 + 37.0 * M + 211.5 * np.arange(n)
    return table(cs, M, iso, nu, 10.0 ** (-24.0 + (np.arange(n) % 5)), 0.06 + 0.003 * np.arange(n), 0.09, 150.0 + 100.0 * np.arange(n), 0.71)


def iso_states():
    return [(T, P, Pp) for T, (P, Pp) in zip(T_ISO, ((2e3, 10.0), (1e5, 4e4), (5e4, 0.0), (3e4, 3e4), (7e2, 70.0)))]


# sixteen members: every gas slot, a different molecule each, three lines per member at interleaved positions (the merged order
# alternates members); members 4 and 5 share the position of their second line (the stable tie of the merge)
N_MEMBERS = 16
CUT_MEMBERS = 2.0
GAP_MEMBERS = 6.5                                # > 2 x the widest cut-off used (3.0): a probe sees at most one line per member
OFF_MEMBERS = (0.0, 0.1, -1.0)
MOLECULES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 19, 23, 26, 31)


def member_tables(cs, n=N_MEMBERS, first=0):
    out = []
    for m in range(first, first + n):
        M = MOLECULES[m % len(MOLECULES)]
        pos = 500.0 + GAP_MEMBERS * (N_MEMBERS * np.arange(3) + m % N_MEMBERS) + 0.37 * (m // N_MEMBERS)
        if m % N_MEMBERS == 5:
            pos[1] = 500.0 + GAP_MEMBERS * (N_MEMBERS + 4)
        niso = int(np.sum(cs.MOLPARAM[M].hascheb))
        iso = [1 + (m + i) % niso for i in range(3)]
        out.append(table(cs, M, iso, pos, 10.0 ** (-22.0 + np.arange(3) + 0.1 * m), 0.05 + 0.004 * m, 0.08 + 0.003 * m, 100.0 + 90.0 * m + 400 * np.arange(3),
                         0.5 + 0.02 * m))
    return out


def member_conc(m):
    """member m's own concentration as a function of (T, P): another Pp and scale at every node for every member"""
    return lambda T, P: min(1.0, (0.002 + 0.0031 * m) * (T / 250.0) ** (0.3 + 0.05 * m) * (1.0 + 0.1 * m * P / 1e5))


def member_grid(tabs):
    return np.unique(np.concatenate([sl.nu[:, None] + np.array(OFF_MEMBERS)[None, :] for sl in tabs]).ravel())


def member_expected(tabs, shapes, cuts, conc, Tk, Pk, nu, c0=C0_GPU):
    """(sum_g C_g sigma_g [K, nnu], bound [K, nnu] relative to it) over the members: conc[g, k]; per point the error bounds of the terms add,
    weighted by the terms"""
    K, n = len(Tk), len(nu)
    tot, err = np.zeros((K, n)), np.zeros((K, n))
    for g, sl in enumerate(tabs):
        lines = [line_of(sl, l) for l in range(len(sl.nu))]
        for i, v in enumerate(nu):
            for l, ln in enumerate(lines):
                if abs(v - ln["nu"]) <= cuts[g] + 1e-9:
                    for k in range(K):
                        w, _, info = sigma_isolated(shapes[g], v, ln, Tk[k], Pk[k], conc[g, k] * Pk[k], cuts[g], conc[g, k])
                        tot[k, i] += w
                        err[k, i] += abs(w) * lineparam_bound(info, c0)
    return tot, err / np.where(tot != 0, np.abs(tot), 1.0)
