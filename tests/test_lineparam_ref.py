"""Host tests of tests/lineparam_ref.py, the 40-digit reference of the per-(state, line) parameter stage: it is held to the oracle
(oracle/cs_oracle.c: shape!, chebyQrefQ; codes 4-6 from its Voigt of one-line tables) at the very probes tests/test_gpu_lineparams.py runs on the
device, to two closed forms and to test_oracle.py's anchors; the constant c0 of its bound is measured here and printed, and the probe
builders are shown to isolate one line per probe."""
import mpmath as mp
import numpy as np
import pytest

import ckdvvh_ref as CK
import lineparam_ref as R
import voigt_lbl_ref as V

ORACLE_SHAPE = {0: "voigt", 1: "lorentz", 2: "doppler"}


def oracle_sigma(cs, O, code, nu, sl, T, P, Pp, cut):
    """the oracle's cross-section of the scalar methods (inclusive cut-off): shape! for codes 0, 1, 2; codes 4, 5, 6 line by line from its
    Voigt of one-line tables (ckdvvh_ref.tilde: S scaled to S / R(nul, T)) -- the profile, the mirror resonance as the even profile at -nu; the pedestal from
    ckdvvh_ref.line_terms -- so that no line's term passes through a sum with another's (strengths here span 50 orders)"""
    if code in ORACLE_SHAPE:
        return O.shape_bang(ORACLE_SHAPE[code], nu, sl, T, P, Pp, cut, strict_ends=False)
    if code & R.PSHIFT:   # line l's term is the unflagged term on the grid nu - s_l (clearsky_hip.h): one-line tables, the grid rounded once
        out = np.zeros(len(nu))
        for l in range(len(sl.nu)):
            out += O.shape_bang(ORACLE_SHAPE[code & ~R.PSHIFT], np.asarray(nu) - sl.delta_a[l] * P / R.KATM, CK.tilde(cs, sl, T, l, l + 1, scale=False),
                                T, P, Pp, cut, strict_ends=False)
        return out
    if code == R.LBL:     # voigt_lbl_ref.expected, the composite the device's code-7 tests use, on one-line tables
        out = np.zeros(len(nu))
        for l in range(len(sl.nu)):
            one = V.subset(sl, np.arange(len(sl.nu)) == l)
            out += V.expected(cs, O, one, sl.delta_a[l:l + 1], nu, T, P, Pp, cut, strict=False)[0]
        return out
    ped, vvh = code in (4, 6), code in (5, 6)
    nu = np.asarray(nu, float)
    out = np.zeros(len(nu))
    voigt = lambda one, x: O.shape_bang("voigt", x, one, T, P, Pp, cut, strict_ends=False)
    for l, nl in enumerate(sl.nu):
        one = CK.tilde(cs, sl, T, l, l + 1, scale=vvh)
        fD = CK.line_terms(cs, O, sl, np.array([cut]), T, P, Pp, [l], vvh)[0] if ped else 0.0   # (at the exact offset: nl + cut rounds)
        term = voigt(one, nu) - fD * ~(np.abs(nu - nl) > cut)
        m = ~(nu + nl > cut) if vvh else np.zeros(len(nu), bool)
        if m.any():
            term[m] += voigt(one, -nu[m][::-1])[::-1] - fD
        out += term * (CK.R(cs, nu, T) if vvh else 1.0)
    return np.maximum(out, 0.0) if ped else out


@pytest.fixture(scope="module")
def shifted(cs, tmp_path_factory):
    return R.shifted_table(cs, tmp_path_factory.mktemp("lineparam"))


def calls(cs, shifted=None):
    """every (table, states, cut, codes) the device tests evaluate one line at a time"""
    out = []
    if shifted is not None:
        for K, seed in ((8, 1), (17, 2)):
            out.append((shifted, R.states(K, seed), R.CUT_EDGE, (17,)))
            out.append((shifted, R.states(K, seed, with_vacuum=True), R.CUT_EDGE, (16, 18, R.LBL)))
    for sl, K, seed in R.edge_tables(cs):
        out.append((sl, R.states(K, seed), R.CUT_EDGE, (1,)))
        out.append((sl, R.states(K, seed, with_vacuum=True), R.CUT_EDGE, (0, 2, 4, 5, 6)))
    for M in sorted(cs.MOLPARAM):
        if np.any(cs.MOLPARAM[M].hascheb):
            out.append((R.iso_table(cs, M), R.iso_states(), R.CUT_ISO, (0, 1, 2)))
    return out


@pytest.fixture(scope="module")
def measured(cs, O, shifted):
    """per code: (worst oracle error / (U x model terms without c0), Faddeeva allowance taken off for Voigt codes; underflow share;
    worst error / bound with C0_ORACLE; probes)"""
    res = {}
    for sl, sts, cut, codes in calls(cs, shifted):
        lines = [R.line_of(sl, l) for l in range(len(sl.nu))]
        for code in codes:
            nu, pr = R.probes(lines, sts, code & ~R.PSHIFT, cut, far=code in (4, 6, R.LBL), centres=R.shifted_centres(sl, sts) if R.shifts(code) else None)
            infos = []
            want, bnd, zero = R.expected(code, sl, sts, nu, pr, cut, c0=R.C0_ORACLE, infos=infos)
            got = np.zeros(len(pr))
            for k, (T, P, Pp) in enumerate(sts):
                s = oracle_sigma(cs, O, code, nu, sl, T, P, Pp, cut)
                for q, (kk, i, l) in enumerate(pr):
                    if kk == k:
                        got[q] = s[i]
            r = res.setdefault(code, dict(ratio=0.0, under=0, n=0, worst=0.0))
            assert np.all(got[zero] == 0.0)
            m = ~zero & (np.abs(want) >= R.UNDERFLOW)
            r["under"] += int(np.sum(~zero & ~m))
            r["n"] += int(np.sum(~zero))
            assert np.all(np.isfinite(got[~zero & ~m]) & (got[~zero & ~m] >= 0) & (got[~zero & ~m] < 1e-289))
            e = np.abs(got[m] - want[m]) / np.abs(want[m])
            r["worst"] = max(r["worst"], float(np.max(e / bnd[m])))
            # the model's terms without c0, from the bound: bound x rel = U (c0 + terms) + F
            t = np.array([(R.model_terms(infos[q]), infos[q]["rel"], R.FADDEEVA if infos[q]["voigt"] else 0.0) for q in np.nonzero(m)[0]])
            ex = np.maximum(e * t[:, 1] - t[:, 2], 0.0) / R.U
            r["ratio"] = max(r["ratio"], float(np.max(ex / t[:, 0])))
            r["c0"] = max(r.get("c0", 0.0), float(np.max(ex - t[:, 0])))
    return res


def test_reference_matches_oracle(measured):
    """the oracle stays within the model with the recorded c0 at every probe of the device tests, every code"""
    for code, r in sorted(measured.items()):
        print(f"code {code}: {r['n']} probes, oracle error / bound(C0_ORACLE = {R.C0_ORACLE}) <= {r['worst']:.3f}, underflow class "
              f"{r['under']} ({100.0 * r['under'] / r['n']:.1f} %)")
        assert r["worst"] <= 1.0, code
        assert r["under"] <= 0.10 * r["n"], code


def test_measure_c0(measured):
    """c0 = the smallest constant with which the model covers the oracle: the worst of error / U - terms (beside it the worst ratio
    error / (U x terms)); the device gets GPU_FACTOR x the recorded value"""
    worst = max(r["c0"] for r in measured.values())
    for code, r in sorted(measured.items()):
        print(f"code {code}: measured c0 {r['c0']:.2f}, ratio (oracle error) / (U x terms without c0) {r['ratio']:.2f}")
    print(f"measured c0 = {worst:.2f}; recorded C0_ORACLE = {R.C0_ORACLE}, GPU factor {R.GPU_FACTOR}, C0_GPU = {R.C0_GPU}")
    assert worst <= R.C0_ORACLE


def test_intensity_at_tref_and_lorentz_integral(cs):
    """at T = Tref the exponential factors cancel: S(Tref) = S Qref/Q(Tref) exactly; the isolated Lorentz profile integrates to
    S(T) (2/pi) atan(cut / gamma) over the cut-off"""
    sl = R.edge_tables(cs)[1][0]
    for l in range(len(sl.nu)):
        ln = R.line_of(sl, l)
        S, _ = R.intensity(ln, 296.0)
        q, _ = R.qrefq(296.0, ln["cheb"])
        assert abs(S / (mp.mpf(ln["S"]) * q) - 1) < mp.mpf(10) ** -38
    ln = R.line_of(sl, 3)
    T, P, Pp, cut = 250.0, 3e4, 1e3, 0.9
    S, _ = R.intensity(ln, T)
    g = R.gamma_lorentz(ln, T, P, Pp)
    c = ln["nu"]
    for v in (c - cut, c - 0.1, c, c + 0.01, c + cut):                      # sigma_isolated is S florentz at the doubles it is given ...
        assert abs(R.sigma_isolated(1, v, ln, T, P, Pp, cut)[1] / (S * R.florentz(mp.mpf(v) - mp.mpf(c), g)) - 1) < mp.mpf(10) ** -38
    assert R.sigma_isolated(1, c + 1.01 * cut, ln, T, P, Pp, cut)[1] == 0
    I = mp.quad(lambda v: S * R.florentz(v, g), [-cut, -0.1, -0.01, 0, 0.01, 0.1, cut])   # ... whose integral over the cut-off is closed
    assert abs(I / (S * 2 / mp.pi * mp.atan(mp.mpf(cut) / g)) - 1) < mp.mpf(10) ** -20   # (the quadrature's own error)


def test_anchors(cs, O, lines):
    """test_oracle.py's anchors of Qref/Q, and the reference's chebyQrefQ against the oracle's for every isotopologue with a fit"""
    sl = lines("CO2")
    a = sl.cheb[0, : sl.ncheb[0]]
    assert float(R.qrefq(296.0, a)[0]) == pytest.approx(0.9987408464004868, rel=1e-14)
    assert float(R.qrefq(250.0, a)[0]) == pytest.approx(1.2273351054954134, rel=1e-14)
    worst = 0.0
    for M, mpar in cs.MOLPARAM.items():
        for i in np.nonzero(mpar.hascheb)[0]:
            a = np.asarray(mpar.cheb[i], float)[: int(mpar.ncheb[i])]
            for T in R.T_EDGE + R.T_ISO:
                q, cond = R.qrefq(T, a)
                worst = max(worst, abs(O.chebyQrefQ(T, a) / float(q) - 1.0) / (R.U * (3.0 + len(a) * cond)))
    print(f"chebyQrefQ: oracle error / (U (3 + n cond)) <= {worst:.3f}")   # (an n-term sum: n roundings on sum |a_k T_k|; 1/y, tau, float(q))
    assert worst <= 1.0


def test_probes_isolate_one_line(cs, shifted):
    """every probe has exactly one line of its table within the cut-off (none for the probe placed beyond it), counted on the host from the
    state's own (shifted) centres, and no other line's mirror resonance (nu + nul <= cut) reaches it"""
    n = 0
    for sl, sts, cut, codes in calls(cs, shifted):
        lines = [R.line_of(sl, l) for l in range(len(sl.nu))]
        for code in codes:
            psh = R.shifts(code)
            cen = R.shifted_centres(sl, sts) if psh else [list(sl.nu)] * len(sts)
            nu, pr = R.probes(lines, sts, code & ~R.PSHIFT, cut, far=code in (4, 6, R.LBL), centres=cen if psh else None)
            assert len(nu) <= 600 and np.all(np.diff(nu) > 0) and nu[0] > 0
            for k, i, l in pr:
                inside = abs(nu[i] - cen[k][l]) <= cut
                assert R.lines_within(cen[k], nu[i], cut) == (1 if inside else 0), (code, k, nu[i])
                assert np.all(np.delete(sl.nu, l) + nu[i] > cut)
                n += 1
    for k, (T, P, Pp) in enumerate(R.FILTER_STATES):       # the end-point case: exact arithmetic, the centre on nu_N + cut at 2 atm only
        c = R.shifted_centres(shifted, R.FILTER_STATES)[k][5]
        assert c == 15000.0 + 0.25 * P / R.KATM and (c == R.FILTER_GRID[-1] + R.FILTER_CUT) == (k == 0) and c <= R.FILTER_GRID[-1] + R.FILTER_CUT
        assert all(R.lines_within(np.delete(shifted.nu, 5), v, R.FILTER_CUT + 30.0) == 0 for v in R.FILTER_GRID)
    tabs = R.member_tables(cs)
    nu = R.member_grid(tabs)
    assert len({sl.M for sl in tabs}) == R.N_MEMBERS
    assert tabs[4].nu[1] == tabs[5].nu[1]
    order = np.argsort(np.concatenate([sl.nu for sl in tabs]), kind="stable") // 3
    assert np.all(order[:4] == [0, 1, 2, 3])           # (the merged order alternates members)
    for sl in tabs:
        for v in nu:
            assert R.lines_within(sl.nu, v, 3.0) <= 1
    print(f"{n} probes, each with one line in reach")
