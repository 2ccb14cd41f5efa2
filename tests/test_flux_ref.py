"""CPU tests of tests/flux_ref.py: the per-element bound of the flux stage is neither too tight nor idle.

  * the oracle's flux stage (O.fluxes_discretized, gray + sigma_extra, no lines) lies within bounds("libm") at factor 1, element by
    element, over every temperature profile and boundary setting of flux_ref, nstream in {1, 2, 4, 7, 9, 16} x nlobatto in {2, 3, 5, 16}
    (24 cases: each (nstream, nlobatto) pair once, each (profile, boundary) pair once; a 25th with two bands).  Measured: worst ratio 0.48.
  * the double restatement passes every case as it is and fails with each planted fault; for every fault there is a case that the new
    comparison rejects and the existing criterion for M+- (1e-11 max M + conftest.source_rounding_bound) accepts.  The existing
    criterion is the one for the fluxes, as test_gpu_flux_orders._vs_oracle applies it; that test's separate 1e-11 relative check of
    tau does see fault "tau" (1e-10 of one optical depth) and "floor" -- their gap is in M+-, where they move elements by far more than
    the bound and far less than 1e-11 of the column maximum.  No fault slips through both.
  * a NaN or an infinity in any one plane, or in a bound, fails the comparison (flux_ref.ratio gives inf, flux_ref.within looks at
    every plane on its own).
  * sharpness, as a condition on the inputs: isothermal cases have bound <= 1e-13 |value| in every compared element, for both
    arithmetics; over the gradient cases at least a quarter of the M+- elements have bound <= 1e-12 |value|.
"""
import numpy as np
import pytest

import flux_ref as F
from conftest import source_rounding_bound

NS, NLOB, PROFILES = (1, 2, 4, 7, 9, 16), (2, 3, 5, 16), ("a", "b", "c")
NNU = 2 * F.D                                  # two periods of the cross-section plane
GRAY = 1e-33                                   # rounds into the plane's last bit: the reference takes the sum the oracle formed
CASES = [(PROFILES[n % 3], F.BOUNDARIES[n // 3], NS[n % 6], NLOB[n // 6]) for n in range(24)]
# case 24, "two bands": a mid-infrared band of deep columns beside the near-infrared one with the full set of columns, no beam, no
# albedo -- the second band's fluxes are ~1e-27 of the first's, so nothing that happens in it reaches 1e-11 of the grid's maximum
CASES.append(("a", ("none", "none", 0.6), 4, 3))
NC = len(CASES)
_IDS = ["%s-%s-%s-%.1f-ns%d-nlob%d" % ((p,) + b + (ns, nl)) for p, b, ns, nl in CASES]
_IDS[24] += "-two-bands"


def test_cases_cover_the_settings():
    assert len({(p, b) for p, b, _, _ in CASES[:24]}) == 24 and len({(ns, nl) for _, _, ns, nl in CASES[:24]}) == 24
    assert {b[0] for b in F.BOUNDARIES} >= {"none", "zero", "pos"} and {b[1] for b in F.BOUNDARIES} >= {"none", "zero", "fun", "one"}
    assert {b[2] for b in F.BOUNDARIES} == {0.0, 0.6, 1.5}


_DONE = {}


def _case(cs, O, n):
    """case n: its inputs, the oracle's outputs, the reference on the cross-sections and quadrature numbers the oracle used"""
    if n not in _DONE:
        prof, (fS, fa, th), ns, nlob = CASES[n]
        kw = {}
        if n == 24:
            kw = dict(nu=np.concatenate([np.linspace(600.0, 760.0, F.D), np.linspace(F.NU_LO, F.NU_HI, F.D)]),
                      sset=np.concatenate([F.S_THICK, F.S_FULL]))
        c = F.case(cs, prof, ns, nlob, nnu=NNU, fS=fS, fa=fa, theta=th, **kw)
        r = O.fluxes_discretized(c["nu"], c["P"], c["g"], nlob, c["Tn"], c["mun"], c["Tlev"], [], [], [], np.zeros((0, c["K"])),
                                 sigma_gray=GRAY, sigma_extra=c["sigma"], S_toa=c["S_toa"], albedo=c["albedo"], theta_s=th, nstream=ns,
                                 want_sigma=True)
        c["sigma"] = r["sigma"]
        c["m"], c["W"] = O.streamnodes(ns)
        c["ws"] = O.lobattonodes(nlob)[1]
        assert F.planck_clear_of_overflow(c)
        ref = F.mp_fluxes(**F.args_of(c), detail=True)
        _DONE[n] = (c, r, ref, F.bounds(ref, "libm"))
    return _DONE[n]


def test_inputs_span_the_regimes(cs):
    """columns from every layer on the floor to ~1e4; layer depths on both sides of the floor, in 1e-6..1e-2, near 1, and past
    tau m_k = 745 for the steepest stream while the shallowest stays below; four decades of depth within one column"""
    c = F.case(cs, "a", 16, 3, nnu=NNU)
    tau = F.np_fluxes(**F.args_of(c))["tau"]
    col = tau.sum(axis=0)
    assert np.all(tau[:, col.argmin()] == 1e-6) and 5e3 < col.max() < 2e4
    assert np.any(tau == 1e-6) and np.any((tau > 1e-6) & (tau < 1e-2)) and np.any((tau > 0.5) & (tau < 2.0))
    assert np.any((tau * c["m"].max() > 745.0) & (tau * c["m"].min() < 745.0))
    thick = tau[:, col.argmax()]
    assert thick.max() / thick.min() > 1e4
    assert np.ptp(c["muk"]) > 0 and 0.5 <= F.f_node(np.arange(c["K"])).min() and F.f_node(np.arange(c["K"])).max() <= 1.5


@pytest.mark.parametrize("n", range(NC), ids=_IDS)
def test_oracle_within_bound(cs, O, n):
    """factor 1, element by element; exact zeros where the reference has them"""
    c, r, ref, b = _case(cs, O, n)
    rr = F.ratios(r, ref, b)
    print("\n  %s: worst error / bound  tau %.3f  M+ %.3f  M- %.3f" % (_IDS[n], rr["tau"], rr["Mup"], rr["Mdn"]))
    assert F.within(rr), rr


@pytest.mark.parametrize("plane", ["tau", "Mup", "Mdn"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_not_finite_is_rejected(cs, O, plane, bad):
    """one NaN or infinity in any output plane fails the comparison, whichever plane it is in; so does a bound that is not finite"""
    c, r, ref, b = _case(cs, O, 2)
    got = {k: np.array(r[k]) for k in ("tau", "Mup", "Mdn")}
    assert F.within(F.ratios(got, ref, b))
    got[plane][-1, 5] = bad
    rr = F.ratios(got, ref, b)
    assert rr[plane] == np.inf and not F.within(rr)
    bb = {k: np.array(b[k]) for k in b}
    bb[plane][0, 0] = bad
    assert not F.within(F.ratios(r, ref, bb))
    assert not F.within(dict(tau=0.3, Mup=float("nan"), Mdn=0.2))


def _old_accepts(cs, c, got, ref):
    """the existing criterion for the fluxes: |M+- - ref| < 1e-11 max M + source_rounding_bound (one number per grid)"""
    d = ref["detail"]
    sm = max(d["Mup"].max(), d["Mdn"].max())
    amp = source_rounding_bound(cs, c["nu"], c["Tlev"], d["tau"])
    return all(np.max(np.abs(got[k] - d[k])) < 1e-11 * sm + amp for k in ("Mup", "Mdn"))


def _applies(fault, n):
    _, (fS, fa, th), ns, _ = CASES[n]
    return not ((fault == "weights" and ns < 2) or (fault == "beam" and (fS in ("none", "zero") or th == 0.0))
                or (fault == "albedo" and fa in ("none", "zero")))


def test_restatement_within_bound(cs, O):
    for n in range(NC):
        c, _, ref, b = _case(cs, O, n)
        rr = F.ratios(F.np_fluxes(**F.args_of(c)), ref, b)
        assert F.within(rr), (_IDS[n], rr)


@pytest.mark.parametrize("fault", F.FAULTS)
def test_planted_fault_rejected(cs, O, fault):
    """the restatement with the fault fails the comparison in at least one case (in fact in every case where the fault changes
    anything: printed), and in at least one of those the existing criterion accepts it; the bound of the device's scan form, the
    loosest in use, rejects it too"""
    rejected, gap, loosest = [], [], []
    for n in range(NC):
        if not _applies(fault, n):
            continue
        c, _, ref, b = _case(cs, O, n)
        got = F.np_fluxes(**F.args_of(c), fault=fault)
        assert all(np.all(np.isfinite(got[k])) for k in got)          # (a rejection below is the fault's, not a NaN's)
        # (the loosest bound the device tests use: the device's exponential, the scan form's chunk roundings)
        if not F.within(F.ratios(got, ref, F.bounds(ref, "device", per=F.scan_per(len(c["P"]) - 1)))):
            loosest.append(n)
        if not F.within(F.ratios(got, ref, b)):
            rejected.append(n)
            if _old_accepts(cs, c, got, ref):
                gap.append(n)
    print("\n  %s: rejected in %d cases, of which the existing criterion accepts %d: %s" % (fault, len(rejected), len(gap),
                                                                                         [_IDS[n] for n in gap[:3]]))
    assert rejected, fault
    assert gap, fault
    assert loosest, fault


def _sharpness(ref, b):
    d = ref["detail"]
    v = np.concatenate([d["Mup"].ravel(), d["Mdn"].ravel()])
    e = np.concatenate([b["Mup"].ravel(), b["Mdn"].ravel()])
    keep = v != 0.0                                   # (M- at the top without a beam is an exact zero on both sides)
    return e[keep] / np.abs(v[keep])


def test_sharpness(cs, O):
    grad = []
    for n in range(NC):
        c, _, ref, b = _case(cs, O, n)
        if CASES[n][0] == "b":
            for arith in ("libm", "device"):
                bb = F.bounds(ref, arith)
                s = _sharpness(ref, bb)
                assert s.max() <= 1e-13, (_IDS[n], arith, s.max())
                assert np.all(bb["tau"] <= 1e-13 * ref["detail"]["tau"])
        elif CASES[n][0] == "a":
            grad.append(_sharpness(ref, F.bounds(ref, "device")))
    grad = np.concatenate(grad)
    frac = float(np.mean(grad <= 1e-12))
    print("\n  gradient cases: %.2f of the M+- elements have bound <= 1e-12 |value|" % frac)
    assert frac >= 0.25
