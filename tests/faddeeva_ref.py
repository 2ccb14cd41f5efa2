"""Re w(x + iy) at 40 digits, a 40-digit restatement of every branch of csrc/cs_faddeeva.h (and of oracle/cs_oracle.c) as written, and the
rounding model of each branch -- shared by tests/test_faddeeva_ref.py (host: the oracle), tests/test_gpu_faddeeva.py (device:
cs_faddeeva_batch) and tests/isolated_line_ref.py (the Faddeeva allowance of the sharp bound below s = 1e4).  Nothing here reads the
oracle or the GPU; c0[] and c1[] are read from the text of cs_faddeeva.h, so that a digit changed there is a digit changed here.

w40(x, y) is Re exp(-z^2) erfc(-iz) from the definition, on the exact double inputs.

restate(x, y, form) runs the operations of fad_re (form "device") or cso_faddeeva_re (form "scalar") once, in the order of the source,
on pairs (value, err): the value at 40 digits with NO rounding -- the double constants of the source taken exactly, pi exact where the
source calls sincospi, the double M_PI where it multiplies by it -- and err, a first-order bound of the absolute error that the double
evaluation of the same operations can have.  The branch and the grid are chosen as the source chooses them, from the double s (the
device: fma(x, x, y * y); the oracle: x * x + y * y) and from frac(2x) in doubles.

  truncation   |value - w40| / w40: what the branch's algorithm (its last term, its node count, its double constants) costs at that
               probe.  Exact; no figure is assumed.
  rounding     err / w40.  Every operation adds U = 2^-53 times the magnitude of its result and carries the errors of its operands with
               the magnitudes of the 40-digit values: a product a b takes |a| e_b + |b| e_a, a sum e_a + e_b, so where a branch
               subtracts (nr bi - ni br; trapezoid sum + pole term; ca dr - sa di; x^2 - y^2) each part counts with |part| / |result|
               and no conditioning constant is guessed.  An fma of the source is counted as a product and a sum (one rounding more than
               it has), which holds whether or not the compiler contracts.
               division        scalar: U (IEEE); the device's 1.0 / s of fad_re's far branch: U
               rcp_nr          U + (2e-15)^2: the first Newton step leaves rcp_nr1's 2e-15, the second squares it and rounds once
               rcp_fast(da db) isolated_line_ref.rcp_fast at the 40-digit da db, per term of fad_near (24 terms of one sign)
               exp             device 2 ulp, libm 1 (lineparam_ref: "Its exp is good to 2 ulp against libm's < 1"), after the
                               argument's own error: -4 pi y carries U 4 pi y, y^2 - x^2 up to U (x^2 + y^2 + |y^2 - x^2|)
               sincospi        2 ulp of each value (the figure taken for the device's exp); libm's sin, cos 1 ulp.  The reduced
                               argument q = 4x - 2 rint(2x) is exact.  The scaled argument (2 / kPi) x y carries two roundings,
                               2 U |2xy| of phase (cs_faddeeva.h states "below 1e-14" for it: |2xy| <= s < 100 gives 2.2e-14 as a
                               bound, which is what is counted); the oracle's 2 x y one, and its M_PI q one
               coefficients    the device's c0[], c1[] are constants (their distance from exp(-t^2) is truncation); the oracle
                               forms them with libm's exp at start-up: U each
  bound(x, y, form) = truncation + rounding, relative to w40.

Vacuum (y = 0).  Below s = 100 fad_near returns the pole term alone, exp(-x^2) to the relative bound.  From s = 100 on both sources
return an exact 0: every term of the continued fraction and of the series carries the factor y.  The true value is exp(-x^2) <=
exp(-100) = 3.8e-44, so the bound there is absolute: got == 0 or |got - w40| <= w40 (`vacuum`).  No probe with y > 0 is held absolutely.

probes() is the structured, seeded set (under 3,000 points): both sides of s = 100, 1e3, 1e4 at 13 angles and four small y; x on and
beside the nodes k / 2 and the grid-choice boundaries k / 2 + 1/8, 3/8; y over the decades from 1e-12 to 9.9 and about 2 pi (the
pole-correction switch); the x where exp(-x^2) = y / (sqrt(pi) x^2), where the two parts of fad_near trade places; negative x; the far
series up to x = 10^7.5, y = 1e4; y = 0 along x = 0 .. 30; a random fill drawn as test_faddeeva_device draws it.

Figures of the model over the probes with y > 0 (host; asserted below 1e-13 by tests/test_faddeeva_ref.py):
  branch      truncation                                      bound, device                              bound, scalar
  far         5.9e-15 (s = 1e4: the fifth term)               6.7e-15                                    6.7e-15
  mid         1.4e-15 (s = 100)                               4.3e-14 at x = 10, y = 1e-10: nr bi - ni    the same
                                                              br cancels to 1/19 of its parts there
  near-int    2.9e-16                                         2.5e-14: 24 x rcp_fast, of one sign         7.5e-15
  near-half   7.6e-15 (x = 6.375, 6.125: the first node       3.4e-14: the same                           2.4e-14 at x -> 10, y = 0: the argument
              left out is 1/8, 3/8 away)                                                                  of exp(y^2 - x^2) carries 2 U x^2
The term that dominates the device's bound is rcp_fast in fad_near (1.4e-14 .. 3.2e-14 per term, all terms of one sign) and, in fad_mid at
small y next to s = 100, the cancellation of nr bi - ni br.  Worst error / bound of the oracle and of the device: see the two test modules.
"""
import functools
import math
import os
import re

import mpmath as mp
import numpy as np

mp.mp.dps = 40
U = 2.0 ** -53
RCP_NR = U + (2e-15) ** 2
EXP_ULP = {"device": 2.0, "scalar": 1.0}
TRIG_ULP = {"device": 2.0, "scalar": 1.0}
K_PI = 3.14159265358979323846                # kPi, M_PI: the same double
K_ISQPI = {"device": 0.5641895835477563, "scalar": 0.56418958354775628695}
FAR_S, MID_S, SER_S = 1.0e4, 100.0, 1.0e3
PA = (180.9375, -330.0, 147.0, -22.0, 1.0)
PB = (-29.53125, 295.3125, -393.75, 157.5, -22.5, 1.0)
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "clearsky.jl_amd", "csrc", "cs_faddeeva.h")


def _coefficients():
    """(c0[13], c1[12]) as the header writes them"""
    with open(HEADER) as f:
        src = f.read()
    out = []
    for name, n in (("c0", 13), ("c1", 12)):
        m = re.search(r"constexpr double %s\[%d\] = \{([^}]*)\}" % (name, n), src)
        v = [float(t) for t in m.group(1).replace("\n", " ").split(",")]
        assert len(v) == n
        out.append(tuple(v))
    return out


C0, C1 = _coefficients()
_f = lambda x: mp.mpf(float(x))


def w40(x, y):
    """Re w(x + iy) = Re exp(-z^2) erfc(-iz) at 40 digits on the exact doubles (mpf)"""
    z = mp.mpc(_f(x), _f(y))
    return (mp.exp(-z * z) * mp.erfc(-1j * z)).real


def w_series(x, y, terms=24):
    """the asymptotic series sum_k (2k-1)!! / 2^k Im(-z^-(2k+1)) ... as i / (sqrt(pi) z) sum_k (2k-1)!! / (2 z^2)^k, for the self-check of
    w40 where it converges to 40 digits (s >= 1e4: the 24th term is below 1e-60)"""
    z = mp.mpc(_f(x), _f(y))
    acc, term = mp.mpc(0), mp.mpc(1)
    for k in range(terms):
        acc += term
        term *= (2 * k + 1) / (2 * z * z)
    return (1j / (mp.sqrt(mp.pi) * z) * acc).real


# ---- (value, err) arithmetic ------------------------------------------------------------------------------------------------------------

NVAR = 768
_n = [0]


class V:
    """a 40-digit value and d[i] = (its derivative by the i-th elementary error of the evaluation) x (that error's largest size): the
    roundings of one evaluation are numbered as they occur, so an error that reaches the result by two ways (a Horner partial sum feeds
    the real and the imaginary part; y^2 feeds all 24 denominators) counts once, with the sign each way gives it.  d = None: exact."""
    __slots__ = ("v", "d")

    def __init__(self, v, d=None):
        self.v, self.d = v, d

    @property
    def e(self):
        return 0.0 if self.d is None else float(np.sum(np.abs(self.d)))


def _c(x):
    return V(_f(x))


def _own(v, d, size):
    """d with one more elementary error of the given absolute size"""
    if size == 0.0:
        return V(v, d)
    d = np.zeros(NVAR) if d is None else d
    d[_n[0]] = size
    _n[0] += 1
    return V(v, d)


def _lin(a, ca, b, cb):
    """ca a.d + cb b.d as a new array (None where both are exact)"""
    if a.d is None and b.d is None:
        return None
    if b.d is None:
        return a.d * ca
    if a.d is None:
        return b.d * cb
    return a.d * ca + b.d * cb


def _add(a, b, exact=False):
    v = a.v + b.v
    return _own(v, _lin(a, 1.0, b, 1.0), 0.0 if exact else U * abs(float(v)))


def _sub(a, b, exact=False):
    v = a.v - b.v
    return _own(v, _lin(a, 1.0, b, -1.0), 0.0 if exact else U * abs(float(v)))


def _mul(a, b, exact=False):
    v = a.v * b.v
    return _own(v, _lin(a, float(b.v), b, float(a.v)), 0.0 if exact else U * abs(float(v)))


def _rcp(a, rel):
    """1 / a by a reciprocal whose own relative error is at most rel"""
    v = 1 / a.v
    return _own(v, None if a.d is None else a.d * -float(v * v), rel * abs(float(v)))


def _exp(a, ulp):
    v = mp.exp(a.v)
    return _own(v, None if a.d is None else a.d * float(v), ulp * U * float(v))


def _sincos(ph, ulp):
    """(sin, cos) of the phase ph (radians, with its errors)"""
    s, c = mp.sin(ph.v), mp.cos(ph.v)
    return (_own(s, None if ph.d is None else ph.d * float(c), ulp * U * abs(float(s))),
            _own(c, None if ph.d is None else ph.d * -float(s), ulp * U * abs(float(c))))


def _rcp_fast(s):
    import isolated_line_ref
    return isolated_line_ref.rcp_fast(float(s))


# ---- the branches -------------------------------------------------------------------------------------------------------------------------

def s_of(x, y, form):
    """the double s of the source: the device's fma(x, x, y * y), the oracle's x * x + y * y"""
    x = abs(float(x))
    y2 = float(y) * float(y)
    return float(_f(x) * _f(x) + _f(y2)) if form == "device" else x * x + y2


def grid_shift(x):
    """fad_near's choice: the half-shifted grid where frac(2x) is more than 1/4 from 1/2"""
    u = 2.0 * abs(float(x))
    return abs((u - math.floor(u)) - 0.5) > 0.25


def branch_of(x, y, form):
    """'far', 'mid', 'near-int' (integer grid) or 'near-half' (half-shifted), as the source decides"""
    s = s_of(x, y, form)
    return "far" if s >= FAR_S else "mid" if s >= MID_S else "near-half" if grid_shift(x) else "near-int"


def _far(x, y, form):
    X, Y = _c(x), _c(y)
    y2 = _mul(Y, Y)
    inv = _rcp(_add(_mul(X, X), y2), U)
    t = _mul(y2, inv)
    h = lambda cs: functools.reduce(lambda acc, c: _add(_mul(acc, t), _c(c)), cs[1:], _c(cs[0]))
    p1 = h((-2.0, 1.5))
    p2 = h((12.0, -15.0, 3.75))
    if form == "device":
        p3 = h((-120.0, 210.0, -105.0, 13.125))
        core = _mul(inv, _add(_mul(inv, _add(_mul(inv, _add(_mul(inv, p3), p2)), p1)), _c(1.0)))
        return _mul(_mul(_c(K_ISQPI[form]), Y), core)
    p3 = _mul(_c(1.875), h((-64.0, 112.0, -56.0, 7.0)))
    inner = _add(p1, _mul(inv, _add(p2, _mul(inv, p3))))
    return _mul(_mul(_mul(_c(K_ISQPI[form]), Y), inv), _add(_c(1.0), _mul(inv, inner)))


def _mid(x, y, form):
    X, Y = _c(x), _c(y)
    ur, ui = _sub(_mul(X, X), _mul(Y, Y)), _mul(_mul(_c(2.0), X, exact=True), Y)

    def horner(cs):
        cr, ci = _c(cs[-1]), _c(0.0)
        for c in cs[-2::-1]:
            tr = _add(_sub(_mul(cr, ur), _mul(ci, ui)), _c(c))
            ci = _add(_mul(cr, ui), _mul(ci, ur))
            cr = tr
        return cr, ci
    ar, ai = horner(PA)
    br, bi = horner(PB)
    nr, ni = _sub(_mul(X, ar), _mul(Y, ai)), _add(_mul(X, ai), _mul(Y, ar))
    num = _sub(_mul(nr, bi), _mul(ni, br))
    den = _rcp(_add(_mul(br, br), _mul(bi, bi)), RCP_NR if form == "device" else U)
    return _mul(_mul(_c(K_ISQPI[form]), num), den)


def _near(x, y, form, parts=None, shift=None):
    X, Y = _c(x), _c(y)
    dev = form == "device"
    shift = grid_shift(x) if shift is None else shift
    y2 = _mul(Y, Y)
    acc = V(mp.mpf(0))
    if not shift:
        acc = _rcp(_add(_mul(X, X), y2), RCP_NR if dev else U)        # (c0[0] = 1)
    for k in range(12):
        t = _c(0.5 * (k + 1) - (0.25 if shift else 0.0))
        c = C1[k] if shift else C0[k + 1]
        a, b = _sub(X, t), _add(X, t)
        da, db = _add(_mul(a, a), y2), _add(_mul(b, b), y2)
        if dev:
            den = _mul(da, db)
            term = _mul(_mul(_c(c), _add(da, db)), _rcp(den, _rcp_fast(den.v)))
        else:
            term = _mul(_own(_f(c), None, U * c), _add(_rcp(da, U), _rcp(db, U)))
        acc = _add(acc, term)
    if dev:
        res = _mul(_mul(_c(0.5 / K_PI), Y), acc)
    else:
        res = _mul(_mul(_mul(_c(0.5), Y, exact=True), _rcp(_c(K_PI), U)), acc)
    if parts is not None:
        parts["sum"] = res.v
    if float(y) < 2.0 * K_PI:
        sgn = 1.0 if shift else -1.0
        g = _exp(_mul(_c(-4.0 * K_PI), Y), EXP_ULP[form])
        q = math.remainder(4.0 * abs(float(x)), 2.0)                    # 4x - 2 rint(2x): exact in doubles
        if dev:
            sph, cph = mp.sinpi(_f(q)), mp.cospi(_f(q))
            sph, cph = _own(sph, None, TRIG_ULP[form] * U * abs(float(sph))), _own(cph, None, TRIG_ULP[form] * U * abs(float(cph)))
            sa, ca = _sincos(_mul(_mul(_mul(_c(2.0 / K_PI), X), Y), V(mp.pi), exact=True), TRIG_ULP[form])
        else:
            sph, cph = _sincos(_mul(_c(K_PI), _c(q)), TRIG_ULP[form])
            sa, ca = _sincos(_mul(_mul(_c(2.0), X, exact=True), Y), TRIG_ULP[form])
        dr = _add(g, _mul(_c(sgn), cph, exact=True))
        di = _mul(_c(-sgn), sph, exact=True)
        em = _exp(_sub(y2, _mul(X, X)), EXP_ULP[form])
        num = _sub(_mul(ca, dr), _mul(sa, di))
        den = _rcp(_add(_mul(dr, dr), _mul(di, di)), RCP_NR if dev else U)
        pole = _mul(_mul(_mul(_mul(_c(2.0), g, exact=True), em), num), den)
        if parts is not None:
            parts["pole"] = pole.v
        res = _add(res, pole)
    return res


@functools.lru_cache(maxsize=None)
def restate(x, y, form="device", branch=None):
    """(branch, 40-digit value of the branch as the source writes it, bound of the absolute rounding error of its double evaluation);
    branch: evaluate that branch ("far", "mid", "near": the grid the source takes, "near-int", "near-half": that grid) instead of the one the
    source takes at (x, y) (the isolated-line allowance near a threshold)"""
    x, y = abs(float(x)), float(y)
    b = branch or branch_of(x, y, form)
    _n[0] = 0
    r = _far(x, y, form) if b == "far" else _mid(x, y, form) if b == "mid" else _near(x, y, form, shift={"near-int": False, "near-half": True}.get(branch))
    return b, r.v, float(r.e)


def near_parts(x, y, form="device"):
    """the two parts of fad_near at 40 digits: {'sum': trapezoid sum, 'pole': pole correction (absent from y = 2 pi on)}"""
    parts = {}
    _n[0] = 0
    _near(abs(float(x)), float(y), form, parts)
    return parts


def vacuum(x, y, form="device"):
    """y = 0 from s = 100 on: the probes held absolutely (module docstring)"""
    return float(y) == 0.0 and s_of(x, y, form) >= MID_S


@functools.lru_cache(maxsize=None)
def terms(x, y, form="device", branch=None):
    """(branch, truncation, rounding), both relative to w40"""
    b, v, e = restate(x, y, form, branch)
    w = w40(abs(float(x)), y)
    return b, float(abs(v - w) / w), float(e / w)


def bound(x, y, form="device", branch=None):
    """relative bound of the source's double Re w at (x, y) against w40: truncation + rounding"""
    _, t, r = terms(x, y, form, branch)
    return t + r


# ---- probes -------------------------------------------------------------------------------------------------------------------------------

SEED = 985
ANGLES = 13
Y_SMALL = (1e-10, 1e-6, 1e-3, 0.1)
Y_GRID = (1e-6, 1e-2, 1.0)
X_POLE = (0.0, 0.3, 1.0, 2.6, 5.2, 7.3)
MAX_PROBES = 3000


def _ulp(v, n):
    for _ in range(abs(n)):
        v = math.nextafter(v, math.inf if n > 0 else -math.inf)
    return v


def crossover(y):
    """the x > 1 where exp(-x^2) = y / (sqrt(pi) x^2) (bisection in doubles; None where y is too large for one)"""
    f = lambda x: -x * x - math.log(y / (math.sqrt(math.pi) * x * x))
    lo, hi = 1.0, 10.0
    if f(lo) <= 0.0 or f(hi) >= 0.0:
        return None
    for _ in range(60):
        m = 0.5 * (lo + hi)
        lo, hi = (m, hi) if f(m) > 0.0 else (lo, m)
    return lo


@functools.lru_cache(maxsize=None)
def probes():
    """(x[n], y[n], kind[n]) -- the structured set of the module docstring, n <= MAX_PROBES, without duplicates"""
    pts = []
    add = lambda x, y, kind: pts.append((float(x), float(y), kind))
    for S in (MID_S, SER_S, FAR_S):
        for rel in (0.0, 1e-9, -1e-9, 1e-3, -1e-3):
            r = math.sqrt(S * (1.0 + rel))
            for j in range(ANGLES):
                th = 0.5 * math.pi * j / (ANGLES - 1)
                x, y = (r * math.cos(th) if j < ANGLES - 1 else 0.0), (r * math.sin(th) if j else 0.0)
                add(x, y, "edge")
                if rel == 0.0:   # one ulp of the larger coordinate to either side: s moves by about an ulp of its own
                    for n in (-1, 1):
                        add(*((_ulp(x, n), y) if x >= y else (x, _ulp(y, n))), "edge")
            for y in Y_SMALL:
                x = math.sqrt(S * (1.0 + rel) - y * y)
                add(x, y, "edge")
                if rel == 0.0:
                    add(_ulp(x, -1), y, "edge")
                    add(_ulp(x, 1), y, "edge")
    for k in range(20):
        for o in (0.0, 0.125, 0.25, 0.375):
            x0 = 0.5 * k + o
            for x in (x0, _ulp(x0, -1), _ulp(x0, 1), x0 - 1e-12, x0 + 1e-12):
                for y in Y_GRID:
                    add(x, y, "grid")
    ys = [10.0 ** e for e in range(-12, 1)] + [9.9, _ulp(2.0 * K_PI, -1), 2.0 * K_PI, _ulp(2.0 * K_PI, 1)]
    for y in ys:
        for x in X_POLE:
            add(x, y, "pole")
    for e in range(-12, 0):
        xc = crossover(10.0 ** e)
        if xc is not None:
            for f in (1.0, 0.95, 1.05):
                add(f * xc, 10.0 ** e, "crossover")
    for e in np.arange(2.0, 7.6, 0.5):
        for y in (1e-6, 1e-2, 1.0, 100.0, 1e4):
            add(10.0 ** e, y, "far")
    for x in (0.0, 1.0, 50.0):
        for y in (100.0, 1e3, 1e4):
            add(x, y, "far")
    for x in list(np.arange(0.0, 30.25, 0.5)) + [_ulp(10.0, -1), 9.99, 10.01]:
        add(x, 0.0, "vacuum")
    rng = np.random.default_rng(SEED)
    for x, y in zip(rng.uniform(0, 12, 400), 10 ** rng.uniform(-10, 1.2, 400)):
        add(x, y, "random")
    for x, y in zip(10 ** rng.uniform(0, 7.5, 300), 10 ** rng.uniform(-6, 4, 300)):
        add(x, y, "random")
    for x, y in zip(-rng.uniform(0, 30, 100), rng.uniform(1e-4, 3, 100)):
        add(x, y, "random")
    seen, out = set(), []
    for p in pts:
        if p[:2] not in seen:
            seen.add(p[:2])
            out.append(p)
    assert len(out) <= MAX_PROBES
    return (np.array([p[0] for p in out]), np.array([p[1] for p in out]), np.array([p[2] for p in out]))


@functools.lru_cache(maxsize=None)
def reference(form):
    """per probe: (w40 as doubles, branch names, truncation, rounding, vacuum mask) under `form`"""
    x, y, _ = probes()
    n = len(x)
    want, br, tr, rd, vac = np.zeros(n), [], np.zeros(n), np.zeros(n), np.zeros(n, bool)
    for i in range(n):
        want[i] = float(w40(abs(x[i]), y[i]))
        vac[i] = vacuum(x[i], y[i], form)
        if vac[i]:
            br.append(branch_of(x[i], y[i], form))
            continue
        b, tr[i], rd[i] = terms(float(x[i]), float(y[i]), form)
        br.append(b)
    return want, np.array(br), tr, rd, vac


def held(got, form, what=""):
    """got[n] at the probes against w40 under bound(., form): returns {branch: (worst error / bound, x, y, error, bound)}; raises
    AssertionError naming the worst probes beyond it.  Vacuum probes: exactly 0, or within w40 of w40."""
    x, y, _ = probes()
    want, br, tr, rd, vac = reference(form)
    got = np.asarray(got, float)
    assert np.all(np.isfinite(got)), what
    assert np.all((got[vac] == 0.0) | (np.abs(got[vac] - want[vac]) <= want[vac])), (what, "vacuum")
    m = ~vac
    assert np.all(want[m] > 1e-290) and np.all((y > 0.0) | vac | (np.array([s_of(a, b, form) for a, b in zip(x, y)]) < MID_S))
    b = tr + rd
    ratio = np.where(m, np.abs(got - want) / np.where(m, want, 1.0) / np.where(m, b, 1.0), 0.0)
    out = {}
    for name in ("far", "mid", "near-int", "near-half"):
        sel = np.nonzero(m & (br == name))[0]
        i = sel[np.argmax(ratio[sel])]
        out[name] = (float(ratio[i]), float(x[i]), float(y[i]), float(ratio[i] * b[i]), float(b[i]))
    bad = np.nonzero(ratio > 1.0)[0]
    worst = [(br[i], float(x[i]), float(y[i]), float(ratio[i] * b[i]), float(b[i])) for i in bad[np.argsort(ratio[bad])[::-1][:6]]]
    assert not len(bad), f"{what}: beyond the bound at {len(bad)} probes, worst (branch, x, y, error, bound): {worst}"
    return out
