"""Far-wing expansion of the Voigt function used by the matrix-core kernels, and the radii where its truncation holds (CPU only; mpmath).

sqrt(pi) K(x,y)/y = sum_{n>=1} c_n(y^2) / x^(2n)   from  K = Re w(x+iy),  w(z) ~ (i/(sqrt(pi) z)) sum_k (2k-1)!!/(2 z^2)^k,
c_n polynomials of degree n-1 in y^2 with rational coefficients (printed; sep_step in cs_kernels.h holds n = 1..8).
The relative truncation error after n terms is below ((y^2 + a_n)/x^2)^n, a_3 = 3.5, a_4 = 3.0, a_8 = 4.4 (the sweep below finds 2.4 / 2.8 /
4.4 enough).  A bound eps then needs (y^2 + a_n)/x^2 <= eps^(1/n); with x = sqrt(ln2) dnu/alpha, y = sqrt(ln2) gamma/alpha that is
    |dnu| >= kSep_n sqrt(gamma^2 + (a_n/ln2) alpha^2),   kSep_n = eps^(-1/(2n))
(sep_radii in cs_kernels.h: kSepEps, kSepR*, kSepA*).  Every line adds a positive term to sigma and the truncation errors of one series
share a sign, so a per-line relative bound eps bounds the relative error of the sum as well.

    python tools/voigt_series.py [--eps 1e-15] [--golden tests/golden/series_radii.json]

prints the coefficients, kSep_n and a_n, sweeps y in [1e-3, 100] along each boundary (and 1.5x / 4x inside it) with the truncation error
and the float64 rounding error of the series as the device evaluates it (series_f64), and with --golden writes the boundary samples with
40-digit values of sqrt(pi) K(x,y)/y (tests/test_series_radii.py).
"""
import argparse
import json
import math
from fractions import Fraction as Fr
from math import comb

A_N = {3: 3.5, 4: 3.0, 8: 4.4}       # the a_n of the bound ((y^2 + a_n)/x^2)^n
SQLN2 = math.sqrt(math.log(2.0))


def coefficients(N=9):
    def dfact(k):
        r = 1
        for q in range(1, 2 * k, 2):
            r *= q
        return r
    coef = {}
    for k in range(0, N + 2):
        a, m = Fr(dfact(k), 2 ** k), 2 * k + 1
        for j in range(1, 2 * N + 3, 2):           # Re[i z^-m] picks the odd powers of (i y/x)
            n, p = (m + j) // 2, (j - 1) // 2
            if n <= N:
                coef[(n, p)] = coef.get((n, p), 0) + a * (-1) ** j * comb(m + j - 1, j) * (-1) ** ((j + 1) // 2)
    return coef


def constants(eps):
    """{n: (kSep_n, alpha factor)} as the device holds them: both rounded UP (kSep to 4 significant digits, a_n/ln2 to 2 decimals)."""
    out = {}
    for n, an in A_N.items():
        r = eps ** (-0.5 / n)
        e = math.floor(math.log10(r)) - 3
        out[n] = (math.ceil(r / 10.0 ** e) * 10.0 ** e, math.ceil(an / math.log(2.0) * 100.0) / 100.0)
    return out


def radius(n, gamma, alpha, const):
    """sep_radii's R_n for (gamma, alpha): float64 in the device's order, with its 1 + 1e-6 safety factor."""
    k, f = const[n]
    return k * math.sqrt(gamma * gamma + f * alpha * alpha) * (1.0 + 1e-6)


def fma(a, b, c):
    return float(Fr(a) * Fr(b) + Fr(c))   # one rounding, as __builtin_fma


def series_f64(nt, y2, dd, dnu):
    """sum_n a_n w^n as sep_step forms it with p3 = 1 (its common factor A y/sqrt(pi)): a_n = id2^n c_n(y^2) in its Horner forms, w^n by
    repeated products, the terms added in order into one accumulator.  id2 = 1/dd^2 and w = 1/dnu^2 are taken correctly rounded (the
    device's reciprocals are within an ulp or two of that)."""
    id2 = 1.0 / (dd * dd)
    w = 1.0 / (dnu * dnu)
    a = []
    Cn = id2
    a.append(Cn)
    Cn *= id2; a.append(Cn * (1.5 - y2))
    Cn *= id2; a.append(Cn * fma(y2, y2 - 5.0, 3.75))
    if nt >= 4:
        Cn *= id2; a.append(Cn * fma(y2, fma(y2, 10.5 - y2, -26.25), 13.125))
    if nt == 8:
        Cn *= id2; a.append(Cn * fma(y2, fma(y2, fma(y2, y2 - 18.0, 94.5), -157.5), 59.0625))
        Cn *= id2; a.append(Cn * fma(y2, fma(y2, fma(y2, fma(y2, 27.5 - y2, -247.5), 866.25), -1082.8125), 324.84375))
        Cn *= id2; a.append(Cn * fma(y2, fma(y2, fma(y2, fma(y2, fma(y2, y2 - 39.0, 536.25), -3217.5), 8445.9375), -8445.9375), 2111.484375))
        Cn *= id2; a.append(Cn * fma(y2, fma(y2, fma(y2, fma(y2, fma(y2, fma(y2, 52.5 - y2, -1023.75), 9384.375), -42229.6875), 88682.34375),
                                         -73901.953125), 15836.1328125))
    acc, wn = 0.0, w
    for n in range(nt):
        acc = fma(a[n], wn, acc)
        wn *= w
    return acc


def samples(eps, ny=25, alphas=(1e-3, 5e-2)):
    """Boundary points (n, y2, dd, dnu) in float64 as the device forms them: a line of Doppler width alpha and y = sqrt(ln2) gamma/alpha
    at exactly its own radius R_n(gamma, alpha)."""
    const = constants(eps)
    out = []
    for n in sorted(A_N):
        for alpha in alphas:
            for i in range(ny):
                y = 10.0 ** (-3.0 + 5.0 * i / (ny - 1))
                gamma = y * alpha / SQLN2
                dd = SQLN2 * (1.0 / alpha)
                out.append((n, (gamma * dd) ** 2, dd, radius(n, gamma, alpha, const)))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--eps", type=float, default=1e-15)
    ap.add_argument("--golden", default=None)
    args = ap.parse_args()
    from mpmath import mp, mpf, erfc, exp, sqrt, pi, re
    mp.dps = 40
    c = coefficients()
    for n in range(1, 9):
        print(n, [str(c[(n, p)]) for p in range(n)], [float(c[(n, p)]) for p in range(n)])
    const = constants(args.eps)
    print(f"eps = {args.eps:g}")
    for n in sorted(A_N):
        print(f"  {n} terms: kSep = {const[n][0]:.6g} (eps^(-1/2n) = {args.eps ** (-0.5 / n):.6f}), a_n = {A_N[n]}, alpha factor {const[n][1]:.2f}")

    def ref(y2, dd, dnu):
        x, y = mpf(dd) * mpf(dnu), sqrt(mpf(y2))
        z = x + 1j * y
        return re(exp(-z * z) * erfc(-1j * z)) * sqrt(pi) / y

    def trunc(nt, y2, x):
        y = sqrt(mpf(y2))
        s = sum(mpf(c[(n, p)].numerator) / c[(n, p)].denominator * y ** (2 * p) / mpf(x) ** (2 * n) for n in range(1, nt + 1) for p in range(n))
        return s / ref(y2, 1.0, x) - 1

    rows = samples(args.eps)
    print("relative error along the boundaries: truncation (exact arithmetic) and the float64 series in the device's order")
    worst = {}
    for n, y2, dd, dnu in rows:
        r = ref(y2, dd, dnu)
        tr = float(abs(trunc(n, y2, mpf(dd) * mpf(dnu))))
        f64 = float(abs(mpf(series_f64(n, y2, dd, dnu)) / r - 1))
        inner = [float(abs(trunc(n, y2, mpf(dd) * mpf(dnu) * s))) for s in (1.5, 4.0)]
        w = worst.setdefault(n, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], tr), max(w[1], f64), max(w[2], *inner)
        if dd < 100.0:
            print(f"  n = {n}, y = {math.sqrt(y2):9.3e}, x = {dd * dnu:10.1f}: truncation {tr:.2e}, float64 {f64:.2e}, "
                  f"1.5x / 4x inside {inner[0]:.1e} / {inner[1]:.1e}")
    for n, (tr, f64, inner) in sorted(worst.items()):
        print(f"  worst, {n} terms: truncation {tr:.3e} (bound {args.eps:g}), float64 {f64:.3e}, inside {inner:.2e}")
        assert tr <= args.eps and inner <= tr
    if args.golden:
        json.dump({"eps": args.eps, "dps": mp.dps,
                   "radii": {str(n): {"kSep": const[n][0], "alpha_factor": const[n][1], "a_n": A_N[n]} for n in sorted(A_N)},
                   "note": "ref = sqrt(pi) K(x,y)/y at x = dd*dnu, y = sqrt(y2), computed exactly from the float64 inputs (tools/voigt_series.py)",
                   "samples": [{"n": n, "y2": y2, "dd": dd, "dnu": dnu, "ref": mp.nstr(ref(y2, dd, dnu), 40, min_fixed=1, max_fixed=0)}
                               for n, y2, dd, dnu in rows]},
                  open(args.golden, "w"), indent=0)
        print("wrote", args.golden, len(rows), "samples")
