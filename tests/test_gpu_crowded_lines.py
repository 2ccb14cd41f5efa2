"""Crowded line sums on the device against 40-digit values, up to the limits of the near-line hand-off (tests/crowded_line_ref.py derives
the tables, probes, bounds and the restated check_near_density; tests/test_crowded_line_ref.py checks on the host what is presupposed).

Every line of a crowd is real: a group is M copies of one line, the reference M x its 40-digit value, so a dropped, doubled or misplaced
line among equals moves the sum by 1 / M -- 2.4e-4 at M = 4095, 0.11 at M = 9 -- against bounds of 1e-14 .. 5e-13 (the isolated-line
bounds by the groups' shares of the sum, plus gamma_(N-1)).  Forms, run_column and the `expect` checks are test_gpu_isolated_line's.

  a  piece thresholds    M on both sides of 8 (vector unit / matrix pieces), 16 (tile nodes of a window end) and 48 (phases), every residue
                         of the 4-line step; two split clusters the piece must count by zone; codes 4, 5, 6
  b  queue windows       M on both sides of one and two windows of the 256-entry queue, 4095 = the 12-bit count; three groups whose
                         tier-0 word spans tier-1 lines; the eight-tiles-per-wave grid; cs_shape_batch and cs_shape_points
  c  the offset field    2^20 - 1 lines in one tile's near zone, the real copies' offset with the top bit of its 20 set
  d  refusals            4096 copies refused (CS_EINVAL, the message names the density) by every entry point for the Voigt codes, accepted
                         and right for Lorentz, Doppler and PHCO2; the merged and the shifted check; what a refusal leaves behind

Recorded figures (MI355X; worst error / bound over the forms of a case, hard | sharp; [sharp]: printed only, M >= 256):
  thr/M7 .. M17        8 forms each   0.048 | 0.307            thr/M47 .. M65      0.047 | 0.274
  thr/split-5+3        8 forms        0.045 | 0.300            thr/split-11+5      0.042 | 0.275
  thr/code4-M9, -M17   2 forms        0.046 | 0.305            thr/code5, code6    0.039 | 0.218   (N = 2 M: every copy's mirror term counts)
  q/M3, M4, M5         5 forms        0.025 | 0.214            q/M255              0.048 | 0.210
  q/M256, M257         5 forms        0.049 | [0.209]          q/M4095             0.171 | [0.241]
  q/three              5 forms        0.072 | [0.255]          q/rep8   1 form     0.053 | [0.242]
  qb/M257-K1 .. K33    batch, points  0.052 | [0.241]          qb/M4095-K1 .. K33  0.173 | [0.237]
  off/batch            0.003 | 0.003, off/col 0.001 | 0.001: N is 2^20 there and gamma_(N-1) = 1.2e-10 is the bound; a lost copy of the three is 0.33
  full/code1           0.074 (Lorentz, hard alone)              full/code2          0.242 (Doppler, hard alone)
  pair/merge, merge off   0.075 | [0.101]                       a resident q/M257 column beside refusals   0.049 | [0.207]
  PHCO2  M = 4095 (hand-off)   0.224 | [0.304]                  M = 4096 (own core)   0.223 | [0.302]     batch and points alike
The near-line pair counts are the reference's own to the pair in every run: q/M4095 21,977,865 in tier 0 and 8,722,350 in tier 1 (M x
5367 and M x 2130), q/three 2,683,500 and 1,065,000, q/rep8 2,210,714 and 1,169,093.  Matrix counters under matrix-cores-2 at M = 7:
node_evals_matrix 0, matrix_evals_3term 0 (direct_evals_matrix = matrix_evals_8term = 28,672: the cores, which one line reaches); at M = 8:
147,968 node, 81,920 direct, 172,032 3-term, 16,384 8-term.  Times: the offset case 1.7 s for its table and references, 0.2 s on the
device for both runs, 1.7 s for the table of one line more and its refusal; no other test above 3.1 s (q/three: three 40-digit
references), the 50 together about 22 s.

Seeded defects (scratch builds, not committed; the 49 tests without the offset case):
  sep_run drops the last line of the final 4-line step of every masked run of k_voigt_edge_mx: 20 fail -- every thr/ case from M = 8 on,
      both splits and all six code cases, already under the hard bound, by 2.9e11 (thr/M65) to 2.0e12 (thr/split-11+5) times the hard bound; thr/M7
      passes (the vector unit keeps its pieces) and so do the fine-grid cases, whose probes no window end serves.
  near_pack stores count - 1: 41 fail -- every comparing test (thr/M7 included: the line core), by 3.7e8 (qb/M4095-K16: one line of 4095
      against 6.6e-13) to 1.6e12 (q/M3) times the hard bound; the 8 that pass are the refusals, Lorentz, Doppler, PHCO2 at 4096 copies
      (k_phco2's own core: no range word) and the shifted pair, which compare no Voigt hand-off.
"""
import time

import numpy as np
import pytest

import clearsky_jl_amd
import crowded_line_ref as X
import isolated_line_ref as I
import lineparam_ref as R
import phco2_line_ref as PH
import test_gpu_isolated_line as T

pytestmark = pytest.mark.gpu

EINVAL = -1
FORMS_A = [T.BY_NAME[n] for n in ("default", "matrix-cores-2", "matrix-cores-0", "ends-at-points", "first-level-1", "interp-off", "far-split-2",
                                  "mx-min-states-1")]
FORMS_B = [T.BY_NAME[n] for n in ("default", "near-two-launches", "matrix-cores-0", "interp-off", "sub-lean-never")]
MATRIX_COUNTERS = ("node_evals_matrix", "direct_evals_matrix", "matrix_evals_3term", "matrix_evals_8term")


@pytest.fixture(scope="module")
def cases(cs):
    return X.Cases(cs)


def column_forms(cs, case, forms, shape="voigt"):
    """every form on one case: {form name: (worst / hard, worst / sharp, work, info)}; failures of bounds and reported forms are collected
    and raised together"""
    case.reference()
    rows, failed = {}, []
    for f in forms:
        r = T.run_column(cs, case, f, shape)
        try:
            hard, sharp = X.compare(case, r["got"], f.model(len(case.sizes)), f"{case.name} {f.name}")
        except AssertionError as e:
            failed.append(f"{f.name}: {e}")
            hard = sharp = float("nan")
        if f.expect is not None and shape == "voigt" and not f.expect(r):
            failed.append(f"{f.name}: reported {T._d(r)} {r['info']}")
        rows[f.name] = (hard, sharp, r["work"], r["info"])
        print(f"{case.name} {f.name}: N up to {int(case.N.max())}, worst error / bound  hard {hard:.3f}  sharp {sharp:.3f}{'' if case.sharp_held else ' (printed only)'}")
    assert not failed, "\n".join(failed)
    return rows


# ---- a. piece thresholds ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", X.M_THRESHOLDS)
def test_piece_thresholds(cs, cases, M):
    """M real copies at col/short-cluster's centre under eight forms, both bounds at every probe; with the matrix forms forced the matrix
    counters are non-zero from M = 8 on, and at M = 7 the vector unit keeps the pieces (no node or 3-term evaluation on the matrix cores:
    what one line alone cannot reach either)"""
    case = cases[f"thr/M{M}"]
    rows = column_forms(cs, case, FORMS_A)
    w = rows["matrix-cores-2"][2]
    print(f"thr/M{M} matrix-cores-2:", {c: w[c] for c in MATRIX_COUNTERS + ("node_evals_matrix_3term",)})
    if M >= 8:
        assert all(w[c] > 0 for c in MATRIX_COUNTERS), {c: w[c] for c in MATRIX_COUNTERS}
    else:
        assert w["node_evals_matrix"] == 0 and w["matrix_evals_3term"] == 0 and w["node_evals_matrix_3term"] == 0, w
    assert rows["matrix-cores-0"][2]["node_evals_matrix"] == 0


@pytest.mark.parametrize("split", X.SPLITS, ids=[f"{a}+{b}" for a, b in X.SPLITS])
def test_split_clusters(cs, cases, split):
    """a + b copies at centres one grid step apart: neither sub-group reaches the threshold their sum sits on (8, 16) -- a piece counts
    the lines of its zone, whatever their centres"""
    case = cases["thr/split-%d+%d" % split]
    rows = column_forms(cs, case, FORMS_A)
    w = rows["matrix-cores-2"][2]
    assert all(w[c] > 0 for c in MATRIX_COUNTERS), {c: w[c] for c in MATRIX_COUNTERS}


CODE_CASES = [(c, M) for c in X.CODES for M in X.M_CODES]


@pytest.mark.parametrize("code,M", CODE_CASES, ids=[f"code{c}-M{M}" for c, M in CODE_CASES])
def test_threshold_codes(cs, cases, code, M):
    """codes 4, 5, 6 with 9 and 17 copies, default and matrix-forced; codes 5 and 6 on col/low-vvh's grid, where every copy's mirror term
    counts (N = 2 M at those probes)"""
    case = cases[f"thr/code{code}-M{M}"].reference()
    assert case.N.max() == (2 * M if code in (5, 6) else M)
    column_forms(cs, case, T.CODE_FORMS, T.NAMES[code])


# ---- b. queue windows and the count field --------------------------------------------------------------------------------------------------------

def _tiers_held(case, rows):
    (lo0, hi0), (lo1, hi1) = case.tier_pairs()
    for name, (_, _, w, _) in rows.items():
        assert lo0 <= w["near_pairs_tier0"] <= hi0 and lo1 <= w["near_pairs_tier1"] <= hi1, (case.name, name, w["near_pairs_tier0"], (lo0, hi0), w["near_pairs_tier1"], (lo1, hi1))
    print(f"{case.name}: near-line pairs tier 0 in [{lo0}, {hi0}], tier 1 in [{lo1}, {hi1}]")


@pytest.mark.parametrize("M", X.M_QUEUE)
def test_queue_windows(cs, cases, M):
    """one group mid-tile on the fine grid, core probes and +-12 steps, under both forms of the near-line pass, without the matrix cores,
    without interpolation and without the lean pass; the near-line pair counts of both tiers are M x the reference's own count"""
    case = cases[f"q/M{M}"]
    rows = column_forms(cs, case, FORMS_B)
    assert rows["default"][3]["near_launches"] == 1 and rows["near-two-launches"][3]["near_launches"] == 2
    _tiers_held(case, rows)


def test_three_groups(cs, cases):
    """100, 300 and 100 copies 60 grid steps apart: at the middle group's points the tier-0 word spans all 500 lines, of which the 300 in
    tier 1 are skipped by the tier-0 pass and summed by the tier-1 pass"""
    case = cases["q/three"].reference()
    assert int(case.N.max()) == sum(X.THREE)
    rows = column_forms(cs, case, FORMS_B)
    _tiers_held(case, rows)


def test_eight_tiles_per_wave(cs, cases):
    """257 copies at both rep_centres of the eight-tiles-per-wave grid (col/fine-rep8's): a lane's run straddles queue windows where a
    wave takes eight tiles in turn"""
    case = cases["q/rep8"]
    rows = column_forms(cs, case, T.REP8_FORMS[:1])
    _tiers_held(case, rows)


BATCH_CASES = [(M, K) for M in X.M_BATCH for K in I.K_SETS]


@pytest.mark.parametrize("M,K", BATCH_CASES, ids=[f"M{M}-K{K}" for M, K in BATCH_CASES])
def test_batch_and_points(cs, cases, M, K):
    """cs_shape_batch and cs_shape_points with 257 and 4095 copies, K = 1, 16, 17, 33 states"""
    case = cases[f"qb/M{M}-K{K}"].reference()
    form = T.BY_NAME["default"]
    Tk, P, Pp = (np.array(x) for x in zip(*I.batch_states(K)))
    ctx = form.context(cs)
    try:
        a = cs.shape_batch(case.tables[0], "voigt", case.nu, Tk, P, Pp, case.cut, ctx)
        b = cs.shape_points(case.tables[0], "voigt", case.nu, Tk, P, Pp, case.cut, ctx)
    finally:
        ctx.close()
    for what, got in (("batch", a), ("points", b)):
        hard, sharp = X.compare(case, got[case.k, case.i], form.model(len(case.sizes)), f"{case.name} {what}")
        print(f"{case.name} {what}: {len(case.pr)} probes, worst error / bound  hard {hard:.3f}  sharp {sharp:.3f} (printed only)")


# ---- c. the offset field ---------------------------------------------------------------------------------------------------------------------------

def test_offset_field(cs, cases):
    """2^20 - 1 lines inside one tile's near zone (fillers of 1e-120, spacing by the restated check), three real copies at the tile's top
    point: their offset first - N0 is 2^19 or more.  cs_shape_batch with K = 2 and a 3-level column; one line more is refused."""
    t0 = time.time()
    case, col = cases["off/batch"].reference(), cases["off/col"].reference()
    t1 = time.time()
    form = T.BY_NAME["default"]
    Tk, P, Pp = (np.array(x) for x in zip(*I.batch_states(2)))
    ctx = form.context(cs)
    try:
        got = cs.shape_batch(case.tables[0], "voigt", case.nu, Tk, P, Pp, case.cut, ctx)
        hard, sharp = X.compare(case, got[case.k, case.i], form.model(len(case.sizes)), "off/batch")
        Pl, Tl, sts = X.small_column_states(cs)
        c = cs.Column(Pl, 9.8, Tl, 0.029, 0.0, 0.0, cs.DirectGas(col.tables[0], I.CONC, col.nu, dnu_cut=col.cut), core=cs.Discretized(3, 2), ctx=ctx)
        assert c.K == col.K and np.array_equal(c.Tk, [s[0] for s in sts]) and np.array_equal(c.Pk, [s[1] for s in sts])
        c.run()
        hc, sc = X.compare(col, c.sigma_nodes()[col.k, col.i], form.model(len(col.sizes)), "off/col")
        t2 = time.time()
        more = X.crowd_table(cs, X.offset_groups(cs, case.nu, more=1))
        with pytest.raises(clearsky_jl_amd.ClearSkyHIPError) as e:
            cs.shape_batch(more, "voigt", case.nu, Tk, P, Pp, case.cut, ctx)
        assert e.value.code == EINVAL and "too dense" in str(e.value) and str(1 << X.FIRST_BITS) in str(e.value)
        again = cs.shape_batch(case.tables[0], "voigt", case.nu, Tk, P, Pp, case.cut, ctx)
        assert np.array_equal(again, got)
    finally:
        ctx.close()
    print(f"off/batch: worst error / bound  hard {hard:.3f}  sharp {sharp:.3f}; off/col: hard {hc:.3f}  sharp {sc:.3f}; tables and references {t1 - t0:.1f} s, "
          f"device runs {t2 - t1:.1f} s, refusal and rerun {time.time() - t2:.1f} s")


# ---- d. refusals and what stands beside them -----------------------------------------------------------------------------------------------------

def _refused(call):
    with pytest.raises(clearsky_jl_amd.ClearSkyHIPError) as e:
        call()
    assert e.value.code == EINVAL and "too dense for the near-line hand-off" in str(e.value) and f"{X.M_REFUSED} within" in str(e.value), str(e.value)
    assert "too dense" in clearsky_jl_amd.lib().cs_last_error().decode()


def _column(cs, ctx, tables, nu, shape="voigt", pshift=False, cut=I.CUT):
    P, Tl, _ = I.column_states(cs)
    concs = I.MERGE_CONCS if len(tables) > 1 else (I.CONC,)
    gases = [cs.DirectGas(sl, c, nu, shape=shape, dnu_cut=cut, pressure_shift=pshift) for sl, c in zip(tables, concs)]
    return cs.Column(P, 9.8, Tl, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, 2), ctx=ctx)


@pytest.mark.parametrize("code", (0, 4, 5, 6))
def test_refused_everywhere(cs, cases, code):
    """4096 copies: CS_EINVAL from cs_shape_batch, cs_shape_points, cs_bake and the column's setup, cs_last_error naming the density;
    after each refusal the same context answers a valid call with the values it gave before"""
    dense, good = cases[f"full/code{code}"], cases["q/M257"]
    shape = T.NAMES[code]
    Tk, P, Pp = (np.array(x) for x in zip(*I.batch_states(16)))
    ctx = T.BY_NAME["default"].context(cs)
    try:
        first = cs.shape_batch(good.tables[0], shape, good.nu, Tk, P, Pp, good.cut, ctx)
        for call in (lambda: cs.shape_batch(dense.tables[0], shape, dense.nu, Tk, P, Pp, dense.cut, ctx),
                     lambda: cs.shape_points(dense.tables[0], shape, dense.nu, Tk, P, Pp, dense.cut, ctx),
                     lambda: cs.Gas(dense.tables[0], I.CONC, dense.nu, cs.AtmosphericDomain((200.0, 320.0), 4, (1.0, 1e5), 4), shape=shape, ctx=ctx),
                     lambda: _column(cs, ctx, dense.tables, dense.nu, shape).run()):
            _refused(call)
            assert np.array_equal(cs.shape_batch(good.tables[0], shape, good.nu, Tk, P, Pp, good.cut, ctx), first)
    finally:
        ctx.close()


def test_refusal_leaves_column_and_baked_table(cs, cases):
    """a resident column, and a table baked before a refused cs_bake into the same slot, give their old results bit for bit"""
    dense, good = cases["full/code0"], cases["q/M257"]
    ctx = T.BY_NAME["default"].context(cs)
    try:
        col = _column(cs, ctx, good.tables, good.nu)
        col.run()
        before = col.sigma_nodes().copy()
        dom = cs.AtmosphericDomain((200.0, 320.0), 4, (1.0, 1e5), 4)
        g = cs.Gas(good.tables[0], I.CONC, good.nu, dom, ctx=ctx)
        raw = g.rawsigma(250.0, 1e3).copy()
        conc = np.full(16, I.CONC)
        nu = clearsky_jl_amd.as_f64(dense.nu)
        _refused(lambda: clearsky_jl_amd.check(clearsky_jl_amd.lib().cs_bake(
            ctx.handle, ctx.slot_of(dense.tables[0]), g.slot, 0, I.CUT, len(nu), clearsky_jl_amd.dptr(nu), dom.nT, clearsky_jl_amd.dptr(clearsky_jl_amd.as_f64(dom.T)),
            dom.nP, clearsky_jl_amd.dptr(clearsky_jl_amd.as_f64(dom.P)), clearsky_jl_amd.dptr(conc), None)))
        assert np.array_equal(g.rawsigma(250.0, 1e3), raw)
        _refused(lambda: cs.shape_batch(dense.tables[0], "voigt", dense.nu, [250.0], [1e3], [10.0], I.CUT, ctx))
        col.run()
        assert np.array_equal(col.sigma_nodes(), before)
        hard, sharp = X.compare(good, before[good.k, good.i], T.BY_NAME["default"].model(len(good.sizes)), "q/M257 beside refusals")
        print(f"resident column after refusals: hard {hard:.3f}  sharp {sharp:.3f}")
    finally:
        ctx.close()


@pytest.mark.parametrize("code", (1, 2))
def test_accepted_lorentz_doppler(cs, cases, code):
    """the table refused for the Voigt codes is accepted for Lorentz and Doppler (no near-line hand-off) and right at the core probes:
    the hard bound (lineparam_bound) plus gamma_4095"""
    case = cases[f"full/code{code}"].reference()
    rows = column_forms(cs, case, T.CODE_FORMS[:1], {1: "lorentz", 2: "doppler"}[code])
    assert int(case.N.max()) == X.M_REFUSED and rows["default"][0] <= 1.0


@pytest.mark.parametrize("M", (X.M_REFUSED - 1, X.M_REFUSED))
def test_phco2_keeps_the_dense_table(cs, M):
    """PHCO2 (cut-off 500, fast path on) does not refuse: its pairs within 3 cm^-1 go through the Voigt kernels while their hand-off takes
    the table (4095 copies) and through k_phco2's own core loop beyond (4096).  phco2_line_ref's "mid-tile" case with M copies of its line:
    M x sigma_isolated(3, ...) under phco2_line_ref's hard bound of the run that serves it, plus gamma_(M-1); cs_shape_batch and cs_shape_points"""
    case = PH.Cases(cs)["mid-tile"].reference()
    sl = X.crowd_table(cs, [(case.lines[0][0]["nu"], M, 1.0)])
    assert np.array_equal(sl.S, np.full(M, PH.S_LINE)) and X.near_density(sl, case.nu, 3.0)["ok"] == (M < X.M_REFUSED)
    run = PH.RUN["default" if M < X.M_REFUSED else "own-core"]        # (what the density rule leaves the default settings with)
    Tk, Pk = (np.array(x) for x in zip(*case.states))
    ctx = PH.RUN["default"].context(cs)
    try:
        a = cs.shape_batch(sl, "PHCO2", case.nu, Tk, Pk, PH.CONC * Pk, case.cut, ctx)
        b = cs.shape_points(sl, "PHCO2", case.nu, Tk, Pk, PH.CONC * Pk, case.cut, ctx)
    finally:
        ctx.close()
    for what, got, strict in (("batch", a, True), ("points", b, False)):
        hard, m, sharp, _ = case.bounds(run, strict=strict)
        g = got[case.k, case.i]
        wh = R.check(g, M * case.want, hard + X.gamma_n(M - 1), case.zero, what=f"PHCO2 M = {M} {what}, hard")
        live = m & (M * case.want >= R.UNDERFLOW)
        ws = float(np.max(np.abs(g[live] - M * case.want[live]) / (M * case.want[live]) / (sharp[live] + X.gamma_n(M - 1))))
        print(f"PHCO2 M = {M} {what}: {len(case.pr)} probes, worst error / bound  hard {wh:.3f}  sharp {ws:.3f} (printed only)")


def test_merged_and_apart(cs, cases):
    """two gases of 2048 copies at one centre: each alone accepted, one merged column group refused, with merging off accepted and right"""
    case = cases["pair/merge"].reference()
    Tk, P, Pp = (np.array(x) for x in zip(*I.batch_states(1)))
    ctx = T.BY_NAME["default"].context(cs)
    try:
        for sl in case.tables:
            assert np.all(np.isfinite(cs.shape_batch(sl, "voigt", case.nu, Tk, P, Pp, case.cut, ctx)))
        _refused(lambda: _column(cs, ctx, case.tables, case.nu).run())
    finally:
        ctx.close()
    rows = column_forms(cs, case, T.MERGE_FORMS[2:])
    assert rows["merge-off"][3]["groups"] == 2 and rows["merge-off"][3]["merge"] == 0


def test_shifted_pair(cs, cases, tmp_path):
    """two groups of 2048 copies, between 2 r0 and 2 r0 + 2 ds apart for the column's largest pressure: accepted without pressure_shift,
    refused with it (the check widens by 2 ds)"""
    sl, dist, ds = X.shifted_pair(cs, tmp_path, cases.fine, cases.fine_mid)
    ctx = T.BY_NAME["default"].context(cs)
    try:
        col = _column(cs, ctx, [sl], cases.fine)
        col.run()
        before = col.sigma_nodes().copy()
        assert np.all(np.isfinite(before)) and before.max() > 0.0
        _refused(lambda: _column(cs, ctx, [sl], cases.fine, pshift=True).run())
        col2 = _column(cs, ctx, [sl], cases.fine)
        col2.run()
        assert np.array_equal(col2.sigma_nodes(), before)
    finally:
        ctx.close()
