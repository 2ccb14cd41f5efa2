"""Every long-grid evaluation form of the Voigt line sum on ISOLATED lines against 40-digit values (tests/isolated_line_ref.py, which
derives the probes and both bounds; tests/test_isolated_line_ref.py checks on the host what is presupposed here).

A probe is within the cut-off of one line only, so what the device returns there is one line's term as one form evaluated it: the 2-, 3-
and 4-term far bodies and the near-zone pass of k_voigt_far, the interpolated wings (k_cheb_nodes, k_cheb_nodes_mx, k_cheb_cascade,
k_cheb_apply_mfma), the window ends on the matrix cores (k_voigt_edge_mx, with and without the 16 tile nodes), the sub-tile cores
(k_voigt_sub, series and lean pass) and the near-line tiers.  Each form is held, at every probe, to lineparam_bound(C0_GPU) (the hard
bound, about 2e-13 for the Voigt codes) and -- every code but Lorentz, at every probe, the line core (s < 1e3: the two tiers of
k_voigt_near<0>, <1> and of k_voigt_near_both, fad_re of k_linesum) included -- to the sharp bound (5e-15 .. 4e-14: the Faddeeva allowance
replaced by the per-form figures of the sources and, below s = 1e4, by the per-probe truncation and rounding of tests/faddeeva_ref.py, plus
the conditioning of interpolated probes).  Mixed precision is not in scope.

Column runs report their form (work()["dispatch"], info()), which is asserted where a setting names one; test_coverage asserts that over
the column runs compared here every evaluation class of cs_column_work is non-zero at least once.  One line alone cannot reach four of
them, for reasons in the code, and a case was added for each:
  node_evals_matrix, node_evals_matrix_3term, matrix_evals_3term   sepzones_body and edgezones_body leave a piece of fewer than 8 lines to
      the vector unit ("too short to be worth a wave's trip"; the tile nodes of k_voigt_edge_mx want 16 lines, its phases 48): the
      "-cluster" cases put 63 ghost lines of 1e-120 times the strength beside every line (isolated_line_ref: Clusters)
  direct_by_body t3_cut   the 3-term zone ends at dQ ~ alpha^(2/3) gamma^(1/3) (zone_compute), a few cm^-1 at 670 cm^-1 even in the
      widest state -- short of the cut-off edge; "col/high" puts the line at 10000 cm^-1, where the Doppler width is 15 times larger and
      the zone passes that edge
Through one line alone (no cluster) run: the far bodies t2, t2_cut, t3, t4_cut and the near-zone pass, k_cheb_nodes (t2, t3, t4), the
cascade and both apply forms, the cores of k_voigt_edge_mx (8 terms) with k_voigt_sub (series and lean pass), and both near-line tiers.

Recorded figures (MI355X; worst error / bound over the forms of a case, hard | sharp):
  col/short            1342 probes 33 forms   0.047 | 0.327        col/short-cluster   0.047 | 0.322
  col/four             2440 probes 33 forms   0.060 | 0.381        col/four-cluster    0.060 | 0.381
  col/long             2444 probes  9 forms   0.048 | 0.416        col/long-cluster    0.048 | 0.416
  col/high             1433 probes  3 forms   0.050 | 0.386
  col/short-merge      1606 probes  3 forms   0.046 | 0.347        (merged, merged with matrix cores forced, merge off)
  col/short-lorentz    1342 probes  2 forms   0.944 | -            (code 1 has no sharp bound: isolated_line_ref)
  col/short-ckd        1342 probes  2 forms   0.046 | 0.309
  col/low-vvh           976 probes  2 forms   0.038 | 0.224
  col/low-ckdvvh        976 probes  2 forms   0.037 | 0.218
  col/low-lbl           982 probes  2 forms   0.573 | 0.595        (code 7: col/low-ckdvvh's line with delta = -0.01, read from a .par file; the
                                                                    sharp bound is code 6's plus the centre term, which leads in the Doppler
                                                                    cores of the thin states -- the oracle composite reaches 0.573 | 0.597 there)
  col/short-shifted    1318 probes  2 forms   0.730 | 0.746
  col/fine             1435 probes  4 forms   0.051 | 0.338        (514 of them in the line core, s < 1e3; one and two near-line launches)
  col/fine-rep8        1303 probes  2 forms   0.045 | 0.333        (885 of them in the line core; 2.75e5 points: eight tiles per wave in k_voigt_near<0>, <1>,
                                                                    two lines whose cores cross a wave's last tile and the grid's ragged last tile)
  cs_shape_batch and cs_shape_points, worst of the placements   0.062 (fine) | 0.347 (between-tiles-1024); exactly-cut (points only)
  0.007 | 0.059; batch/fine (342 probes in the line core) 0.062 | 0.340; two P = 0 states through cs_shape_points 0.246, exact 0 from s = 100 on
With the sharp bound on every probe (it began at s = 1e3 before) no ratio above moved but col/short-shifted's, whose worst probe is now one
of the line core.  The line core alone (s < 1e3: fad_mid and fad_near in the near-line kernels, fad_re in k_linesum; worst error / sharp
bound): col/short, -cluster, -merge 0.103; col/four 0.174; col/long 0.144; col/high 0.349; col/short-ckd 0.137; col/low-vvh, -ckdvvh
0.053; col/low-lbl 0.595; col/short-shifted 0.746; col/fine 0.196; col/fine-rep8 0.289; batch/fine 0.276; batch/mid-tile 0.196; the other placements 0.061 and less.
A seeded defect in the line core (c1[1] of fad_near raised by 1e-13, a scratch build): every Voigt case here fails the sharp bound, by
up to 2.63, and none the hard bound -- tests/test_gpu_faddeeva.py has the record.
With rcp_fast at the 3e-15 its header first claimed, the sharp ratios were 0.7 .. 0.98 and, with interpolation off, 1.04 .. 1.21 at
three probes (col/four, col/high): the finding isolated_line_ref describes.

A seeded defect (a scratch build with kSepR4 halved, not committed): col/short-cluster and col/four-cluster fail the sharp bound in
every form that keeps the 4-term matrix pieces -- by 1.09 with all levels on, by 4.3 with first_level 2 (1.5e-13 against 3.9e-14 at
15 cm^-1 from the line in state 47) -- and nothing passes the hard bound; the cases of one line alone pass, since no 4-term matrix piece
serves them (see Clusters).  Of the dense-table tests (series_radii, interp, fuzz, sub_lean: 88) every oracle comparison at 1e-11
passes; two comparisons of the matrix path with the vector path at 2e-14 see 3.1e-14.
"""
import numpy as np
import pytest

import clearsky_jl_amd
import isolated_line_ref as I
import lineparam_ref as R

pytestmark = pytest.mark.gpu

NAMES = {0: "voigt", 1: "lorentz", 4: "voigtCKD", 5: "voigtVVH", 6: "voigtCKDVVH", 7: "voigtLBL"}
FLAGS = clearsky_jl_amd.DISPATCH_FLAGS
COVERAGE = (("direct_by_body", "t2"), ("direct_by_body", "t2_cut"), ("direct_by_body", "t3"), ("direct_by_body", "t3_cut"),
            ("direct_by_body", "t4_cut"), ("direct_by_body", "near_zone"), ("node_by_body", "t2"), ("node_by_body", "t3"),
            ("node_by_body", "t4"), "node_evals_matrix", "direct_evals_matrix", "matrix_evals_3term", "matrix_evals_8term",
            "node_evals_matrix_3term", "sub_evals", "sub_lean_evals", "near_pairs_tier0", "near_pairs_tier1")


@pytest.fixture(scope="module")
def cases(cs, tmp_path_factory):
    d = tmp_path_factory.mktemp("isolated")
    return I.Cases(cs, R.shifted_table(cs, d), I.low_shifted_table(cs, d))


class Form:
    """the settings of one run: mc (cs_set_matrix_cores), interp, first (first_level), tune {key: value}, merge; model: the RunForm the
    sharp bound takes; expect: what the library must report of the run (r = dict(work, info))"""

    def __init__(self, name, mc=2, interp=True, first=0, tune=None, merge=True, expect=None):
        self.name, self.mc, self.interp, self.first, self.tune, self.merge, self.expect = name, mc, interp, first, dict(tune or {}), merge, expect

    def model(self, nlev):
        return I.RunForm(matrix=self.mc != 0, interp=self.interp and self.first < nlev, margin=0.01 * self.tune.get(3, 30), first=self.first,
                         cascade=self.tune.get(12, 0) != 2)

    def context(self, cs):
        ctx = cs.Context(0)
        ctx.set_interp(self.interp)
        ctx.set_interp_plan(first_level=self.first)
        if self.mc is not None:
            ctx.set_matrix_cores(self.mc)
        ctx.set_merge(self.merge)
        for k, v in self.tune.items():
            ctx.set_tuning(k, v)
        return ctx


def _d(r):
    return r["work"]["dispatch"]


_flag = lambda n: (lambda r: bool(_d(r)["flags"] & FLAGS[n]))
_nflag = lambda n: (lambda r: not _d(r)["flags"] & FLAGS[n])
_mx_off = lambda r: _d(r)["tables"] == 0 and r["work"]["node_evals_matrix"] == 0 and r["work"]["direct_evals_matrix"] == 0
_mx_on = lambda r: r["work"]["direct_evals_matrix"] > 0 and r["work"]["matrix_evals_8term"] > 0       # (one line reaches the cores only)
_direct = lambda r: r["work"]["node_evals"] == 0 and r["work"]["node_evals_matrix"] == 0 and r["work"]["direct_evals"] > 0

# every form of the issue's list; the short grid needs cs_set_matrix_cores(2) to reach the matrix forms (an isolated line is far below
# the line density edge_in_use asks for), so 2 is the base of the cs_set_tuning rows
FORMS = [
    Form("default", mc=None),
    Form("matrix-cores-0", mc=0, expect=_mx_off),
    Form("matrix-cores-2", expect=_mx_on),
    # (| 4: no core is handed to the sub-tiles or to the matrix pipe -- EdgeArgs::core = 0 -- and the tile-wide near-zone pass keeps it;
    #  the piece tables are still made)
    Form("matrix-cores-2|4", mc=6, expect=lambda r: _d(r)["tables"] != 0 and r["work"]["sub_evals"] == 0 and r["work"]["matrix_evals_8term"] == 0
         and r["work"]["core_tile_states"] == 0 and r["work"]["direct_by_body"]["near_zone"] > 0),
    Form("interp-off", interp=False, expect=_direct),
    Form("interp-off-vector", mc=0, interp=False, expect=lambda r: _direct(r) and _mx_off(r)),
    Form("first-level-1", first=1),
    Form("first-level-2", first=2),
    Form("first-level-1-vector", mc=0, first=1, expect=_mx_off),
    Form("near-plane-off", tune={7: 0}, expect=lambda r: not _d(r)["streams"] & 2),
    Form("near-plane-on", tune={7: 2}, expect=lambda r: bool(_d(r)["streams"] & 2)),
    Form("far-pieces-64", tune={11: 1}),
    Form("cascade-always", tune={12: 1}),
    Form("cascade-never", tune={12: 2}),
    Form("nodes-split-always", tune={13: 1}, expect=lambda r: _d(r)["nodes_split"] == 1),
    Form("nodes-split-never", tune={13: 2}, expect=lambda r: _d(r)["nodes_split"] == 0),
    Form("nodes-split-never-vector", mc=0, tune={13: 2}, expect=lambda r: _d(r)["nodes_split"] == 0 and _mx_off(r)),
    Form("edge-all-subtiles", tune={14: 1}),
    Form("far64-shared", tune={17: 1}, expect=_flag("FAR64_SHARED")),
    Form("sub-lean-never", tune={18: 1}, expect=lambda r: r["work"]["sub_lean_evals"] == 0),
    Form("sub-lean-first", tune={18: 2}),
    Form("near-two-launches", tune={16: 4}, expect=lambda r: r["info"]["near_launches"] == 2),
    Form("near-memset", tune={7: 2, 19: 1}, expect=_flag("NEAR_MEMSET")),
    Form("tables-own-launch", tune={21: 1}, expect=lambda r: _d(r)["tables"] == 2),
    Form("tables-merged", tune={21: 2}, expect=lambda r: _d(r)["tables"] == 1),
    Form("far-split-1", tune={22: 1}, expect=lambda r: _d(r)["far_split"] == 1),
    Form("far-split-2", tune={22: 2}, expect=lambda r: _d(r)["far_split"] == 2),
    Form("far-split-4", tune={22: 4}, expect=lambda r: _d(r)["far_split"] == 4),
    Form("ends-at-points", tune={23: 1}, expect=_nflag("TNODES")),
    Form("mx-min-states-1", tune={8: 1}),
    Form("mx-min-states-16", tune={8: 16}),
    Form("margin-15", tune={3: 15}),
    Form("margin-100", tune={3: 100}),
]
# No `expect` where the library reports nothing that names the key: keys 3 (margin), 8 (states a matrix piece asks for), 11, 12, 14
# and 18 = 2 have no field in work()["dispatch"] or info() (CASCADE_ASIDE is also set by the fused short-grid apply, whatever key 12 says;
# key 14 changes issued flops on one-wave-per-item grids only).  Their effect on the work counters is asserted where the code fixes its
# direction: test_column_forms compares mx-min-states-1 / default / 16, and the levels carried to the grid under first-level-1 and -2.
BY_NAME = {f.name: f for f in FORMS}
_merged = lambda r: r["info"]["merge"] == 1 and r["info"]["groups"] == 1 and r["info"]["max_members"] == 2 and r["info"]["lines"] == 2
MERGE_FORMS = [Form("merged", mc=None, expect=_merged), Form("merged-matrix-cores-2", expect=_merged),
               Form("merge-off", merge=False, expect=lambda r: r["info"]["merge"] == 0 and r["info"]["groups"] == 2 and r["info"]["max_members"] == 1)]
CODE_FORMS = [BY_NAME[n] for n in ("default", "matrix-cores-2")]
LONG_FORMS = [BY_NAME[n] for n in ("default", "matrix-cores-2", "matrix-cores-0", "ends-at-points", "far-split-2", "nodes-split-always",
                                   "cascade-never", "sub-lean-never", "margin-15")]


def run_column(cs, case, form, shape="voigt", pshift=False):
    """one 61-state column of the case's gases under the form's settings: the cross-sections at the probes, work() and info()"""
    P, T, sts = I.column_states(cs)
    ctx = form.context(cs)
    try:
        concs = I.MERGE_CONCS if len(case.tables) > 1 else (I.CONC,)
        gases = [cs.DirectGas(sl, c, case.nu, shape=shape, dnu_cut=case.cut, pressure_shift=pshift) for sl, c in zip(case.tables, concs)]
        col = cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, 2), ctx=ctx)
        assert col.K == case.K and np.array_equal(col.Tk, [s[0] for s in sts]) and np.array_equal(col.Pk, [s[1] for s in sts])
        assert np.array_equal(col.conc, np.array(concs)[:, None] * np.ones(col.K))
        col.run()                # (a whole step: the dispatch record is the step's)
        return dict(got=col.sigma_nodes()[case.k, case.i], work=col.work(), info=col.info())
    finally:
        ctx.close()


_STORE = {}     # case name -> rows and failures of column_forms


def column_forms(cs, cases, name, forms, shape="voigt", pshift=False):
    """every form on one case: [(form name, worst / hard, worst / sharp, work)], and the failures (bounds, reported forms) as text.
    Kept per case name, so the coverage test reads what the comparing tests ran."""
    store = _STORE.setdefault(name, {})
    if store:
        return store["rows"], store["failed"]
    case = cases[name].reference()
    rows, failed = [], []
    for f in forms:
        r = run_column(cs, case, f, shape, pshift)
        try:
            hard, sharp = I.compare(case, r["got"], f.model(len(case.sizes)), f"{name} {f.name}")
        except AssertionError as e:
            failed.append(f"{f.name}: {e}")
            hard = sharp = float("nan")
        if f.expect is not None and shape == "voigt" and not pshift and not f.expect(r):   # (the matrix pieces are Voigt's, unshifted)
            failed.append(f"{f.name}: reported {_d(r)} {r['info']}")
        rows.append((f.name, hard, sharp, r["work"]))
        store.setdefault("info", {})[f.name] = r["info"]
        store.setdefault("core", {})[f.name] = I.core_ratio(case, r["got"], f.model(len(case.sizes)))
        print(f"{name} {f.name}: worst error / bound  hard {hard:.3f}  sharp {sharp:.3f}")
    store["rows"], store["failed"] = rows, failed
    ok = [x for x in rows if x[1] == x[1]]
    if ok:
        print(f"{name}: {len(case.pr)} probes, {len(forms)} forms; worst over forms  hard {max(x[1] for x in ok):.3f}  sharp {max(x[2] for x in ok):.3f}"
              f"  (line core, s < 1e3: {max(store['core'].values()):.3f})")
    return rows, failed


HIGH_FORMS = [BY_NAME[n] for n in ("default", "matrix-cores-2", "interp-off-vector")]
# the line core on a grid of a third of a Doppler width per point: both forms of the near-line pass, with and without the sub-tile cores
FINE_FORMS = [BY_NAME[n] for n in ("default", "near-two-launches", "matrix-cores-0", "interp-off")]
# eight tiles per wave in k_voigt_near<0>, <1> (voigt_plan: nrep = 8, which has no switch but the grid): two launches whatever key 16 says
_rep8 = lambda r: r["info"]["near_launches"] == 2 and r["work"]["near_pairs_tier0"] > 0 and r["work"]["near_pairs_tier1"] > 0
REP8_FORMS = [Form("default", mc=None, expect=_rep8), Form("near-plane-off", tune={7: 0}, expect=lambda r: _rep8(r) and not _d(r)["streams"] & 2)]
COLUMN_CASES = [("col/short", FORMS, "voigt", False), ("col/four", FORMS, "voigt", False), ("col/long", LONG_FORMS, "voigt", False),
                ("col/short-cluster", FORMS, "voigt", False), ("col/four-cluster", FORMS, "voigt", False),
                ("col/long-cluster", LONG_FORMS, "voigt", False), ("col/high", HIGH_FORMS, "voigt", False),
                ("col/short-merge", MERGE_FORMS, "voigt", False), ("col/short-lorentz", CODE_FORMS, "lorentz", False),
                ("col/short-ckd", CODE_FORMS, "voigtCKD", False), ("col/low-vvh", CODE_FORMS, "voigtVVH", False),
                ("col/low-ckdvvh", CODE_FORMS, "voigtCKDVVH", False), ("col/low-lbl", CODE_FORMS, "voigtLBL", False),
                ("col/short-shifted", CODE_FORMS, "voigt", True),
                ("col/fine", FINE_FORMS, "voigt", False), ("col/fine-rep8", REP8_FORMS, "voigt", False)]


@pytest.mark.parametrize("name,forms,shape,pshift", COLUMN_CASES, ids=[c[0] for c in COLUMN_CASES])
def test_column_forms(cs, cases, name, forms, shape, pshift):
    """a 61-state column (1 Pa .. 3e6 Pa) of isolated lines under every form: eight of its states at every probe, both bounds; the short
    grid (40 tiles and one point, matrix forms forced), the four-level grid (cascade by default), the long grid (one wave per item in
    k_voigt_edge_mx, tile nodes included, and in k_cheb_nodes_mx; far_split 1), a merged second gas, and codes 1, 4, 5, 6, 7 and
    0 | CS_SHAPE_PSHIFT on the default and the matrix-forced form"""
    case = cases[name]
    assert len(case.pr) <= I.MAX_PROBES
    rows, failed = column_forms(cs, cases, name, forms, shape, pshift)
    if name in ("col/long", "col/long-cluster"):
        d = {n: x for n, _, _, x in rows}["matrix-cores-2"]["dispatch"]
        assert d["far_split"] == 1 and d["flags"] & FLAGS["TNODES"] and d["nodes_split"] == 0, d
    if name in ("col/four", "col/four-cluster"):
        assert rows[0][3]["levels"] == 4 and rows[0][3]["intervals"] == I.n_itot(case.sizes, len(case.nu))
    w = {n: x for n, _, _, x in rows}
    if forms is FORMS:
        # first_level = n skips the n largest sizes: the carry to the grid is one contraction per level in use (work(): apply_flops)
        nlev = len(case.sizes)
        for n in (1, 2):
            assert w[f"first-level-{n}"]["apply_flops"] * nlev == w["matrix-cores-2"]["apply_flops"] * (nlev - n) > 0, (name, n)
        # the fewer states a matrix piece asks for (key 8), the longer it is (sepzones_body's rank selection): never fewer evaluations
        assert w["mx-min-states-1"]["node_evals_matrix"] >= w["matrix-cores-2"]["node_evals_matrix"] >= w["mx-min-states-16"]["node_evals_matrix"], name
    if name == "col/short-merge":   # (the merged table is what was compared: one group of two members; apart: two groups)
        assert len(case.tables) == 2 and [f.name for f in forms] == ["merged", "merged-matrix-cores-2", "merge-off"]
    assert not failed, "\n".join(failed)


def test_coverage(cs, cases):
    """over the Voigt column runs compared above, every evaluation class cs_column_work counts is non-zero in at least one run"""
    seen = {}
    for name, forms, shape, pshift in COLUMN_CASES[:7]:
        for fname, _, _, w in column_forms(cs, cases, name, forms, shape, pshift)[0]:
            for c in COVERAGE:
                v = w[c[0]][c[1]] if isinstance(c, tuple) else w[c]
                if v > 0:
                    seen.setdefault(c, f"{name} {fname}")
    for c in COVERAGE:
        print(c, "first non-zero in", seen.get(c))
    assert not [c for c in COVERAGE if c not in seen]
    # the line core under the sharp bound in both forms of the near-line pass: k_voigt_near_both (one launch: the default) and
    # k_voigt_near<0> + <1> (two: cs_set_tuning key 16 | 4), each with pairs in both tiers and compared at probes of both tiers
    for name, forms, least in (("col/short", FORMS, 4), ("col/four", FORMS, 4), ("col/fine", FINE_FORMS, 200)):
        case = cases[name]
        column_forms(cs, cases, name, forms)
        m, _ = case.sharp(BY_NAME["default"].model(len(case.sizes)))
        core0, core1 = int(np.sum(m & (case.s >= 100.0) & (case.s < 1e3))), int(np.sum(m & (case.s < 100.0)))
        rows = {n: (h, sh, w) for n, h, sh, w in _STORE[name]["rows"]}
        for fname, launches in (("default", 1), ("near-two-launches", 2)):
            h, sh, w = rows[fname]
            assert _STORE[name]["info"][fname]["near_launches"] == launches, (name, fname, _STORE[name]["info"][fname])
            assert w["near_pairs_tier0"] > 0 and w["near_pairs_tier1"] > 0 and sh == sh and min(core0, core1) >= least, (name, fname, core0, core1)
        print(f"{name}: {core0} probes with 100 <= s < 1e3, {core1} with s < 100 under the sharp bound, in one and in two near-line launches")


VAC_X = (0.0, 0.3, 1.0, 2.5, 5.0, 7.3, 9.9, 9.999, 10.001, 10.5, 15.0, 20.0, 25.7, 26.5, 40.0)
X_ROUNDINGS = 6.0


def test_points_vacuum_state(cs):
    """cs_shape_points with P = 0 states beside one at 1e4 Pa: y = 0, the profile is exp(-x^2) x sqrt(ln 2 / pi) / alpha.  Points at
    x = VAC_X on both sides of the centre, placed with each vacuum state's own alpha.

    Why not a seventh placement of test_batch_and_points: lineparam_ref.check knows two classes besides the relative one -- `zero` (no
    term within the cut-off) and UNDERFLOW (below 1e-290) -- and a vacuum state's values between |x| = 10 and 25.7 are neither: they lie
    between 1e-61 and 1e-290 of a cm^2, and the device returns an exact 0 there (cs_faddeeva.h: every term of fad_mid and of the series
    carries the factor y).  So the rule is this test's own: from s = 100 on, got == 0 or |got - want| <= want; below, the sharp bound
    with one more term, the Doppler-like conditioning 2 x^2 of the exponent on x = d (sqrt(ln 2) / alpha): alpha carries 3 U
    (lineparam_bound: "alpha = (nul / c) sqrt(2 R T / mu) carries 3 U"), the constant, the quotient and the product one each --
    X_ROUNDINGS = 6, so 12 U x^2, 1.3e-13 at x = 9.999.  (With P > 0 the same term is bounded by 12 U x^2 at the x where the Gaussian
    core ends, 3 to 5 for the states of this suite: a few 1e-15, which the cases above leave inside c0 and the allowance.)"""
    c = I.placements()["mid-tile"][0]
    sl = I.one_line_table(cs, c)
    ln = R.line_of(sl, 0)
    sts = [(296.0, 0.0, 0.0), (200.0, 0.0, 0.0), (296.0, 1e4, 100.0)]
    nu = np.unique([c + sg * x * R.widths(ln, T, P, Pp)[0] / I.SQLN2 for T, P, Pp in sts[:2] for x in VAC_X for sg in (-1.0, 1.0)])
    T, P, Pp = (np.array(v) for v in zip(*sts))
    form = BY_NAME["default"]
    ctx = form.context(cs)
    try:
        got = cs.shape_points(sl, "voigt", nu, T, P, Pp, I.CUT, ctx)
    finally:
        ctx.close()
    model = form.model(3)
    n_rel = n_abs = 0
    worst = 0.0
    for k, (Tk, Pk, Ppk) in enumerate(sts):
        for i, v in enumerate(nu):
            want, _, f = R.sigma_isolated(0, v, ln, Tk, Pk, Ppk, I.CUT)
            x, y = abs(v - c) * I.SQLN2 / f["alpha"], f["gamma"] * I.SQLN2 / f["alpha"]
            assert (y == 0.0) == (Pk == 0.0) and abs((x * x + y * y) / 100.0 - 1.0) > 1e-6
            if y == 0.0 and x * x >= 100.0:
                assert got[k, i] == 0.0 or abs(got[k, i] - want) <= want, (k, x, got[k, i], want)
                assert got[k, i] == 0.0, (k, x, got[k, i])        # today's behaviour, as cs_faddeeva.h states it
                n_abs += 1
                continue
            assert want > R.UNDERFLOW
            b = I.U * (R.C0_GPU + R.model_terms(f) + (2.0 * X_ROUNDINGS * x * x if y == 0.0 else 0.0)) + model.allowance(x, y)
            r = abs(got[k, i] - want) / want / b
            assert r <= 1.0, (k, x, y, got[k, i], want, r * b, b)
            worst = max(worst, r)
            n_rel += 1
    assert n_abs >= 2 * 2 * 7 - 2 and n_rel >= 2 * 2 * 8 - 2 + len(nu)
    print(f"vacuum states: {n_rel} probes under the relative bound (worst error / bound {worst:.3f}), {n_abs} with y = 0 from s = 100 on: exact 0")


BATCH = [(p, f) for p in list(I.placements()) + ["low-vvh", "fine"] for f in ("default", "matrix-cores-2")]


@pytest.mark.parametrize("place,fname", BATCH, ids=[f"{p}-{f}" for p, f in BATCH])
def test_batch_and_points(cs, cases, place, fname):
    """one line per call through cs_shape_batch and cs_shape_points (the same far machinery on the 2561-point grid; the scalar methods'
    inclusive end points in the latter) at the seven placements, state sets of K = 1, 16, 17, 33 (a full state group, a padded group
    of one); "fine": the same point count at a third of a Doppler width per point, whose probes about the centre are the line core"""
    case = cases[f"batch/{place}"].reference()
    form = BY_NAME[fname]
    assert len(case.pr) <= I.MAX_PROBES and case.K in I.K_SETS
    sts = I.batch_states(case.K)
    T, P, Pp = (np.array(x) for x in zip(*sts))
    ctx = form.context(cs)
    try:
        a = cs.shape_batch(case.tables[0], NAMES[case.code], case.nu, T, P, Pp, case.cut, ctx)
        b = cs.shape_points(case.tables[0], NAMES[case.code], case.nu, T, P, Pp, case.cut, ctx)
    finally:
        ctx.close()
    ib = case.i
    if place == "exactly-cut":   # the line at nu_1 - cut, every value dyadic: the strict end-point pre-filter drops it from the vector method
        assert np.all(a == 0.0) and np.sum(~case.zero) == len(case.ksel) and np.all(b[case.k, ib][~case.zero] > 0.0)
    else:
        hard, sharp = I.compare(case, a[case.k, case.i], form.model(len(case.sizes)), f"{place} {fname} batch")
        print(f"batch/{place} {fname}: {len(case.pr)} probes, worst error / bound  hard {hard:.3f}  sharp {sharp:.3f}"
              f"  (line core, s < 1e3: {I.core_ratio(case, a[case.k, case.i], form.model(len(case.sizes))):.3f})")
    hard, sharp = I.compare(case, b[case.k, ib], form.model(len(case.sizes)), f"{place} {fname} points")
    print(f"points/{place} {fname}: worst error / bound  hard {hard:.3f}  sharp {sharp:.3f}")
