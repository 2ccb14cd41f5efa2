"""Host tests of tests/faddeeva_ref.py: the oracle's Re w (oracle/cs_oracle.c: the scalar form of the three branches, IEEE divisions, libm) is
held to bound(., "scalar") against 40-digit values at every probe before the device meets bound(., "device")
(tests/test_gpu_faddeeva.py), and the helper is checked against itself: its branch and grid choices, its truncation figures, its 40-digit
values against the committed goldens and against a second formula, the coefficients it reads from cs_faddeeva.h.

Recorded figures (this project's oracle, glibc's libm; worst error / bound, the probe, error against bound):
  far         0.927 at (100.049988, 1e-06)    6.19e-15 against 6.68e-15
  mid         0.176 at (31.638426, 0.1)       6.84e-15 against 3.89e-14
  near-int    0.384 at (2.87407342, 5.1e-08)  1.26e-15 against 3.28e-15
  near-half   0.792 at (6.125, 1e-06)         7.59e-15 against 9.59e-15
The device's and oracle's s fall on different sides of a threshold at 2 of the 2,618 probes (fma); each is held in the branch it takes.
With c1[1] of cs_faddeeva.h raised by 1e-13 (the seeded defect of tests/test_gpu_faddeeva.py), test_coefficients_of_the_header fails and
test_truncation_and_bounds sees a truncation of 7.1e-14 -- without a GPU.
"""
import math
from fractions import Fraction as Q

import mpmath as mp
import numpy as np

import faddeeva_ref as F


def test_probe_set():
    """the set is what the module says: under MAX_PROBES, every kind and every branch present, both sides of each threshold, both grids on
    both sides of frac(2x) = 1/4 and 3/4, y on both sides of 2 pi, negative x, y = 0 on both sides of s = 100"""
    x, y, kind = F.probes()
    assert 2000 < len(x) <= F.MAX_PROBES and len(set(zip(x, y))) == len(x)
    assert set(kind) == {"edge", "grid", "pole", "crossover", "far", "vacuum", "random"}
    s = np.array([F.s_of(a, b, "device") for a, b in zip(x, y)])
    for S in (F.MID_S, F.SER_S, F.FAR_S):
        for lo, hi in ((1 - 2e-3, 1 - 1e-4), (1 - 2e-9, 1 - 1e-10), (1 - 1e-14, 1.0), (1.0, 1 + 1e-14), (1 + 1e-10, 1 + 2e-9), (1 + 1e-4, 1 + 2e-3)):
            assert np.sum((s >= S * lo) & (s <= S * hi) & (y > 0)) >= 4, (S, lo, hi)
        assert np.any(s == S)
    br = np.array([F.branch_of(a, b, "device") for a, b in zip(x, y)])
    assert all(np.sum((br == b) & (y > 0)) > 300 for b in ("far", "mid", "near-int", "near-half"))
    fr = 2 * np.abs(x) - np.floor(2 * np.abs(x))
    for q in (0.25, 0.75):     # exactly on the boundary (integer grid: |fr - 1/2| > 1/4 is false there) and one ulp to either side
        assert np.any(fr == q) and np.any((fr < q) & (fr > q - 1e-14)) and np.any((fr > q) & (fr < q + 1e-14))
    assert np.any(x < 0) and np.any(y == 2 * F.K_PI) and np.any(y == math.nextafter(2 * F.K_PI, 0)) and np.any(y == math.nextafter(2 * F.K_PI, 7))
    assert np.sum((y == 0) & (s < F.MID_S)) >= 20 and np.sum((y == 0) & (s >= F.MID_S)) >= 40
    assert y.min() == 0.0 and y[y > 0].min() <= 1e-12 and x.max() >= 10 ** 7.5 and y.max() >= 1e4


def test_branch_and_grid_as_the_source():
    """the restatement takes the branch s dictates -- s formed as each source forms it -- and the grid frac(2x) dictates"""
    x, y, _ = F.probes()
    differ = 0
    for form in ("device", "scalar"):
        _, br, _, _, vac = F.reference(form)
        for i in range(len(x)):
            ax, s = abs(float(x[i])), F.s_of(x[i], y[i], form)
            want = "far" if s >= 1e4 else "mid" if s >= 100 else "near"
            assert br[i].split("-")[0] == want, (form, x[i], y[i], s, br[i])
            if want == "near":      # in exact rationals: the integer grid from 1/8 off its nearest node k / 2 on, the half-shifted one nearer
                dist = abs(Q(ax) - Q(round(2 * ax), 2))     # than that -- but for the one rounding of fr - 1/2 in the source's test
                if dist >= Q(1, 8) or dist < Q(1, 8) - Q(1, 2 ** 54):
                    assert br[i] == ("near-int" if dist >= Q(1, 8) else "near-half"), (x[i], dist, br[i])
            assert vac[i] == (y[i] == 0.0 and s >= 100.0)
    dev, sca = F.reference("device")[1], F.reference("scalar")[1]
    differ = int(np.sum(dev != sca))
    # the two sources round s differently (fma): at a threshold's own ulp they may part; each is held in the branch it takes
    print(f"probes where the device's s and the oracle's fall on different sides of a threshold: {differ}")
    assert differ <= 40
    # s exactly representable cases
    assert F.s_of(6.0, 8.0, "device") == 100.0 == F.s_of(6.0, 8.0, "scalar") and F.branch_of(6.0, 8.0, "device") == "mid"
    assert F.branch_of(math.nextafter(10.0, 0), 0.0, "device") == "near-half" and F.branch_of(100.0, 0.0, "scalar") == "far"
    # (one ulp below 1/8 the double fr - 1/2 rounds to 1/4 exactly and the integer grid is still taken, its node 1/8 - 1.4e-17 away)
    assert F.grid_shift(0.125) is False and F.grid_shift(math.nextafter(0.125, 0)) is False and F.grid_shift(0.125 - 1e-12) is True
    assert F.grid_shift(0.375) is False
    assert F.grid_shift(math.nextafter(0.375, 1)) is True and F.grid_shift(0.25) is False and F.grid_shift(0.0) is True


def test_coefficients_of_the_header():
    """c0[k] = exp(-(k/2)^2), c1[k] = exp(-((k + 1/2)/2)^2) of cs_faddeeva.h are the doubles nearest the 40-digit values; PA, PB are the
    convergents of the 10-term continued fraction (exact small rationals: the recurrence in rationals gives them back)"""
    for k, c in enumerate(F.C0):
        assert c == float(mp.exp(-mp.mpf(k * 0.5) ** 2)), ("c0", k)
    for k, c in enumerate(F.C1):
        assert c == float(mp.exp(-mp.mpf((k + 0.5) * 0.5) ** 2)), ("c1", k)
    # z / (z^2 - 1/2 / (1 - 1 / (z^2 - 3/2 / (1 - ...)))) in u = z^2: A_n / B_n by the three-term recurrence of w = (i / sqrt pi) / (z - (1/2) /
    # (z - 1 / (z - (3/2) / (z - ...)))); ten terms, as polynomials in u with z factored out
    pm = lambda p, q: [sum(p[i] * q[j - i] for i in range(len(p)) if 0 <= j - i < len(q)) for j in range(len(p) + len(q) - 1)]
    pa = lambda p, q: [(p[i] if i < len(p) else 0) + (q[i] if i < len(q) else 0) for i in range(max(len(p), len(q)))]
    # convergents of 1 / (z - a1 / (z - a2 / ...)), a_k = k / 2: P_n = z P_{n-1} - a_{n-1} P_{n-2}; as polynomials in z
    P0, P1 = [Q(0)], [Q(1)]
    Q0, Q1 = [Q(1)], [Q(0), Q(1)]
    for n in range(1, 10):
        a = Q(n, 2)
        P0, P1 = P1, pa(pm([Q(0), Q(1)], P1), [-a * c for c in P0])
        Q0, Q1 = Q1, pa(pm([Q(0), Q(1)], Q1), [-a * c for c in Q0])
    # P_10 = z PA(z^2), Q_10 = PB(z^2)
    assert all(c == 0 for c in P1[0::2]) and all(c == 0 for c in Q1[1::2])
    assert [float(c) for c in P1[1::2]] == list(F.PA) and [float(c) for c in Q1[0::2]] == list(F.PB)


def test_w40(golden):
    """w40 reproduces tests/golden/faddeeva.npz to the doubles' own rounding, and the asymptotic series summed to 40 digits where that
    converges (s >= 1e4) -- two formulas, one value"""
    g = golden("faddeeva")
    worst = 0.0
    for x, y, w in zip(g["x"], g["y"], g["w"]):
        v = F.w40(abs(x), y)
        if w > 1e-290:
            worst = max(worst, float(abs(v - mp.mpf(float(w))) / v))
        else:
            assert float(v) < 1e-289
    assert worst <= 2.0 ** -53, worst
    x, y, _ = F.probes()
    n, worst = 0, 0.0
    for a, b in zip(x, y):
        if b > 0 and F.s_of(a, b, "device") >= 1e4:
            worst = max(worst, float(abs(F.w_series(abs(a), b) / F.w40(abs(a), b) - 1)))
            n += 1
    # (w40 takes the real part of a complex product up to sqrt(s) / y = 1e13 times larger: 40 - 13 digits are its own)
    assert n > 300 and worst < 1e-24, (n, worst)
    assert float(F.w40(10.0, 0.0)) == float(mp.exp(-100)) and abs(float(F.w40(0.0, 1e-12)) - 1.0) < 2e-12


def test_truncation_and_bounds():
    """what the module claims of its own figures: truncation below 1e-14 at every probe with y > 0 and at y = 0 below s = 100 (every
    probe but the vacuum ones); the device bound below 1e-13 there; the parts of fad_near trade places at the crossover probes; the
    pole term is absent from y = 2 pi on"""
    x, y, kind = F.probes()
    for form in ("device", "scalar"):
        want, br, tr, rd, vac = F.reference(form)
        m = ~vac
        assert np.all(m[y > 0]) and np.all(want[m] > 1e-290)
        for b in ("far", "mid", "near-int", "near-half"):
            s = m & (br == b)
            i, j = np.nonzero(s)[0][np.argmax(tr[s])], np.nonzero(s)[0][np.argmax((tr + rd)[s])]
            print(f"{form} {b}: {int(s.sum())} probes, truncation <= {tr[i]:.2e} at ({x[i]:.6g}, {y[i]:.3g}), bound <= {(tr + rd)[j]:.2e} at ({x[j]:.6g}, {y[j]:.3g})")
        assert np.max(tr[m]) < 1e-14, (form, np.max(tr[m]))
        assert np.max((tr + rd)[m]) < 1e-13, (form, np.max((tr + rd)[m]))
        assert np.min((tr + rd)[m]) >= 2.0 ** -53
    n = 0
    for i in np.nonzero((kind == "crossover") & (y <= 1e-3))[0][::3]:
        p = F.near_parts(x[i], y[i])
        # exp(-x^2) against y / (sqrt(pi) x^2): equal but for the wing's next term, 3 / (2 x^2) of it (y <= 1e-3: x >= 2.9)
        assert 0.75 < float(p["pole"] / p["sum"]) < 1.25, (x[i], y[i], p)
        n += 1
    assert n >= 10
    assert "pole" not in F.near_parts(0.3, 2 * F.K_PI) and "pole" in F.near_parts(0.3, math.nextafter(2 * F.K_PI, 0))


def test_oracle_within_scalar_bound(O):
    """the oracle's faddeeva at every probe: within bound(., "scalar") of w40 where y > 0 or s < 100; at y = 0 from s = 100 on an exact 0
    (or within w40 of w40 <= 3.8e-44): the vacuum statement of cs_faddeeva.h"""
    x, y, _ = F.probes()
    got = O.faddeeva(x, y)
    out = F.held(got, "scalar", "oracle")
    for b, (r, px, py, err, bnd) in out.items():
        print(f"oracle {b}: worst error / bound {r:.3f} at ({px:.9g}, {py:.3g}): error {err:.2e}, bound {bnd:.2e}")
    vac = F.reference("scalar")[4]
    assert np.all(got[vac] == 0.0) and vac.sum() >= 40          # today's behaviour, which the header now states
    near0 = (y == 0) & ~vac
    assert np.all(got[near0] > 0.0)
