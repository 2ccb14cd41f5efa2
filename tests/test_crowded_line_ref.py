"""Host tests of tests/crowded_line_ref.py: what tests/test_gpu_crowded_lines.py presupposes is checked here without a GPU -- the tables hold
the multiplicities their names give, the restated check_near_density gives every case the verdict it was built for (and the other one a
line further where the case sits at a limit), N is the count of lines_within at every probe, the fillers' part of a sum stays below
1e-100, no probe is of the underflow class -- and the oracle (oracle/cs_oracle.c, O.shape_bang) is held to the same M x 40-digit
reference with RunForm(scalar=True) plus gamma_(N-1) before the device meets it.

The oracle is not run on the million-line table of the offset case (2^20 lines x 134 points x 2 states in scalar code is most of a
minute): its reference is the same three real copies' as everywhere, and its fillers' share is bounded here.

Recorded figures (worst oracle error / bound, hard | sharp; [sharp]: printed only, M >= 256):
  thr/M7 .. M17        0.025 | 0.427            thr/M47 .. M65         0.026 | 0.296
  thr/split-5+3        0.021 | 0.348            thr/split-11+5         0.024 | 0.328
  thr/code4-M9, -M17   0.023 | 0.408            thr/code5, code6       0.007 | 0.111
  q/M3, M4, M5         0.035 | 0.634            q/M255                 0.048 | 0.282
  q/M256, M257         0.048 | [0.281]          q/M4095                0.171 | [0.244]
  q/three              0.141 | [0.604]          q/rep8                 0.053 | [0.317]
  qb/M257-K1 .. K33    0.050 | [0.269]          qb/M4095-K1 .. K33     0.170 | [0.244]
  pair/merge           0.083 | [0.112]          full/code1 0.249, full/code2 0.243 (Lorentz, Doppler: the hard bound alone)
"""
import numpy as np
import pytest

import crowded_line_ref as X
import isolated_line_ref as I
import lineparam_ref as R


@pytest.fixture(scope="module")
def cases(cs):
    return X.Cases(cs)


def _mult(sl):
    return dict(zip(*(a.tolist() for a in np.unique(sl.nu, return_counts=True))))


def test_tables_hold_what_the_cases_name(cs, cases):
    """group multiplicities per case; the M sets lie on both sides of 8, 16 and 48 with every residue of the 4-line step, and on both
    sides of one queue window per lane (64 lanes x 4 = CS_NEAR_Q), of a second window and at the last count the field holds"""
    assert {M % 4 for M in X.M_THRESHOLDS} == {0, 1, 2, 3}
    for t in (8, 16, 48):
        assert {t - 1, t, t + 1} <= set(X.M_THRESHOLDS)
    assert X.NEAR_Q == 64 * 4 and {3, 4, 5, X.NEAR_Q - 1, X.NEAR_Q, X.NEAR_Q + 1, (1 << X.COUNT_BITS) - 1} == set(X.M_QUEUE)
    for M in X.M_THRESHOLDS:
        assert _mult(cases[f"thr/M{M}"].tables[0]) == {cases.mid: M}
    for a, b in X.SPLITS:      # neither sub-group reaches a threshold the sum does: 5 + 3 = 8, 11 + 5 = 16
        c = cases[f"thr/split-{a}+{b}"]
        assert _mult(c.tables[0]) == {cases.mid: a, float(cases.short[20 * 64 + 33]): b} and max(a, b) < a + b and a + b in (8, 16)
    for code in X.CODES:
        for M in X.M_CODES:
            c = cases[f"thr/code{code}-M{M}"]
            assert c.code == code and _mult(c.tables[0]) == {cases.mid if code == 4 else I.LOW_CENTRE: M}
    for M in X.M_QUEUE:
        assert _mult(cases[f"q/M{M}"].tables[0]) == {cases.fine_mid: M} and cases.fine_mid == cases.fine[20 * 64 + 32]
    c = cases["q/three"]
    h = float(c.nu[1] - c.nu[0])
    cen = sorted(_mult(c.tables[0]))
    assert [_mult(c.tables[0])[v] for v in cen] == list(X.THREE) and cen[1] == cases.fine_mid
    assert all(abs((b - a) / h - X.THREE_STEPS) < 1e-6 for a, b in zip(cen, cen[1:]))
    c = cases["q/rep8"]        # the eight-tiles-per-wave rule holds with this table's line count too
    n = len(c.nu)
    assert _mult(c.tables[0]) == {v: 257 for v in I.rep_centres(c.nu)} and I.rep_rules(n - 1, 2 * 257) and not I.rep_rules(n - 2, 2 * 257)
    for M in X.M_BATCH:
        for K in I.K_SETS:
            c = cases[f"qb/M{M}-K{K}"]
            assert c.K == K and c.concs is None and _mult(c.tables[0]) == {cases.fine_mid: M}
    c = cases["pair/merge"]
    assert [_mult(sl) for sl in c.tables] == [{cases.fine_mid: X.M_REFUSED // 2}] * 2 and c.concs == list(I.MERGE_CONCS)
    for name in cases.names() + ["pair/merge", "full/code1", "full/code2"]:
        c = cases[name]
        assert 0 < len(c.pr) <= I.MAX_PROBES and sorted(set(c.k.tolist())) == [k for k in I.STATES_COMPARED if k < c.K], name


def test_restated_check_gives_the_intended_verdicts(cs, cases, tmp_path):
    """every case to be run is accepted by near_density; the count field: 4095 copies accepted with npt = 4095, 4096 refused; two gases of
    2048 accepted each and refused as one merged table; the shifted pair accepted with ds = 0 and refused with the column's ds; the issue's
    figures of amax, r0 and dA on the fine grid"""
    lim = 1 << X.COUNT_BITS
    for name in cases.names():
        c = cases[name]
        d = X.near_density(c.tables[0], c.nu, c.cut)
        cen = [v for v, _, _ in c.real]
        together = max(cen) - min(cen) <= 2.0 * d["r0"]          # (q/three, the splits: one range word spans every group; q/rep8: two far apart)
        assert d["ok"] and d["npt"] == (sum(M for _, M, _ in c.real) if together else c.M_max) and together == (name != "q/rep8"), (name, d)
    d = X.near_density(cases["q/M4095"].tables[0], cases.fine, I.CUT)
    assert d["npt"] == d["nzone"] == lim - 1 and d["ok"]
    assert abs(d["amax"] / 1.42e-3 - 1) < 5e-3 and abs(d["r0"] / 0.0544 - 1) < 5e-3 and abs(d["dA"] / 0.170 - 1) < 5e-3
    for code in (0, 4, 5, 6, 1, 2):
        d = X.near_density(cases[f"full/code{code}"].tables[0], cases.fine, I.CUT)
        assert d["npt"] == lim and not d["ok"]
    c = cases["pair/merge"]
    each = [X.near_density(sl, c.nu, c.cut) for sl in c.tables]
    merged = X.near_density(X.crowd_table(cs, c.gases[0] + c.gases[1]), c.nu, c.cut)
    assert all(e["ok"] and e["npt"] == lim // 2 for e in each) and not merged["ok"] and merged["npt"] == lim
    sl, dist, ds = X.shifted_pair(cs, tmp_path, cases.fine, cases.fine_mid)
    r0 = each[0]["r0"]
    assert 2 * r0 < dist < 2 * r0 + 2 * ds and abs(ds * R.KATM / (X.SHIFT_DELTA * max(P for _, P in cases.column())) - 1.0) < 1e-12
    plain, shifted = X.near_density(sl, cases.fine, I.CUT), X.near_density(sl, cases.fine, I.CUT, ds * (1.0 + 1e-12))
    assert plain["ok"] and plain["npt"] == lim // 2 and not shifted["ok"] and shifted["npt"] == lim


def test_offset_case(cs, cases):
    """the offset field: 2^20 - 1 lines inside span + 2 dA with npt below 2^12, accepted; one filler more refused; the real copies' offset from
    any line at or above the tile's first point minus dA -- where a near zone can start -- has its top bit set; the fillers' share of every
    probe's sum is below 1e-100 of a real line's term; probes: the group's core, +-12 steps, the tile's first and last point"""
    for name in ("off/batch", "off/col"):
        c = cases[name]
        sl = c.tables[0]
        d = X.near_density(sl, c.nu, c.cut)
        assert d["ok"] and d["nzone"] == (1 << X.FIRST_BITS) - 1 == len(sl.nu) and d["npt"] < 1 << X.COUNT_BITS, d
        top = float(c.nu[127])
        first = int(np.searchsorted(sl.nu, top, "left"))
        assert np.all(sl.nu[first:first + X.OFFSET_REAL] == top) and sl.nu[first + X.OFFSET_REAL] > top and c.M_max == X.OFFSET_REAL
        assert first - int(np.searchsorted(sl.nu, c.nu[64], "left")) >= 1 << (X.FIRST_BITS - 1) and first < 1 << X.FIRST_BITS
        assert sl.nu[0] >= c.nu[64] - d["dA"] and sl.nu[-1] <= c.nu[127] + d["dA"]
        share = c.ghost_share()
        assert 0.0 < share < 1e-100 and sum(M for _, M, _ in c.ghosts) == len(sl.nu) - X.OFFSET_REAL
        pts = set(c.i.tolist())
        assert {64, 127} | set(range(127 - X.STEPS12, 127 + X.STEPS12 + 1)) <= pts and sorted(set(c.k.tolist())) == list(range(c.K))
        c.reference()
        within = {i: R.lines_within(sl.nu, c.nu[i], c.cut) for i in set(c.i.tolist())}
        assert np.array_equal(c.N, [within[i] for i in c.i.tolist()]) and c.N.max() > 1 << (X.FIRST_BITS - 1)
        assert not c.zero[c.i == 127].any() and c.zero[c.i == 64].all()      # (the tile's first point is beyond the real copies' cut-off: fillers alone)
        print(f"{name}: {len(sl.nu)} lines, nzone {d['nzone']} npt {d['npt']}, real copies at line {first}, {len(c.pr)} probes, fillers' share {share:.1e}")
    more = X.near_density(X.crowd_table(cs, X.offset_groups(cs, cases['off/batch'].nu, more=1)), cases["off/batch"].nu, I.CUT)
    assert not more["ok"] and more["nzone"] == 1 << X.FIRST_BITS and more["npt"] < 1 << X.COUNT_BITS


def test_counts_and_classes(cs, cases):
    """N at every probe is lines_within over the whole table (a mirror term of codes 5, 6 counts again); the expected value is the groups'
    multiplicities times one line's; no probe of any case is of the underflow class; gamma_(N-1) against (N - 1) U"""
    for name in ("thr/M9", "thr/split-11+5", "thr/code5-M17", "thr/code6-M9", "q/three", "q/M4095", "pair/merge"):
        c = cases[name].reference()
        cen = c.all_centres()
        mirror = c.code in (5, 6)
        for q in range(0, len(c.pr), 7):
            v = c.nu[c.i[q]]
            n = R.lines_within(cen, v, c.cut)
            assert c.N[q] == n + (len(cen) if mirror and v + cen[0] <= c.cut else 0), (name, q)
        if mirror:
            assert np.any(c.N == 2 * c.M_max) and np.any(c.N == c.M_max)
        one = [p.want for p, _ in c.parts]
        assert np.array_equal(c.want, np.sum([M * w for w, (_, M) in zip(one, c.parts)], axis=0))
        assert R.split(c.want[~c.zero])[1] == 0.0, name
        assert np.all(c.gamma >= (c.N - 1).clip(0) * X.U) and np.all(c.gamma <= (c.N - 1).clip(0) * X.U * (1 + 1e-9))
    assert cases["q/M4095"].sharp_held is False and cases["q/M255"].sharp_held is True and cases["q/M256"].sharp_held is False
    (lo0, hi0), (lo1, hi1) = cases["q/M5"].tier_pairs()
    assert 0 < lo0 <= hi0 and 0 < lo1 <= hi1 and lo0 % 5 == 0 and hi1 % 5 == 0


def _oracle(cs, O, c):
    """the oracle's values at the probes of a case: per compared state on the probed points alone (inclusive cut-off), sum over the gases
    of concentration x shape!"""
    import test_lineparam_ref as TL
    pts = np.unique(c.i)
    col = np.searchsorted(pts, c.i)
    got = np.zeros(len(c.pr))
    for k in sorted(set(c.k.tolist())):
        T, P = c.states[k]
        s = sum((1.0 if c.concs is None else c.concs[g]) * TL.oracle_sigma(cs, O, c.code, c.nu[pts], sl, T, P, c.fracs[g] * P, c.cut)
                for g, sl in enumerate(c.tables))
        m = c.k == k
        got[m] = s[col[m]]
    return got


FAMILIES = {
    "thresholds": [f"thr/M{M}" for M in X.M_THRESHOLDS],
    "splits-and-codes": [f"thr/split-{a}+{b}" for a, b in X.SPLITS] + [f"thr/code{c}-M{M}" for c in X.CODES for M in X.M_CODES],
    "queue": [f"q/M{M}" for M in X.M_QUEUE] + ["q/three"],
    "rep8": ["q/rep8"],
    "batch": [f"qb/M{M}-K{K}" for M in X.M_BATCH for K in I.K_SETS],
    "beside-the-refusals": ["pair/merge", "full/code1", "full/code2"],
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_oracle_meets_the_crowd_bounds(cs, O, cases, family):
    """the oracle on every case but the million-line table: within the hard bound (C0_ORACLE) plus gamma_(N-1) at every probe, and within
    the sharp bound of the scalar form plus gamma_(N-1) below SHARP_M copies (printed from there on)"""
    for name in FAMILIES[family]:
        c = cases[name].reference()
        hard, sharp = X.compare(c, _oracle(cs, O, c), I.RunForm(scalar=True, interp=False), name, c0=R.C0_ORACLE)
        print(f"{name}: {len(c.pr)} probes, N up to {int(c.N.max())}, oracle error / bound  hard {hard:.3f}  sharp {sharp:.3f}{'' if c.sharp_held else ' (printed only)'}")
