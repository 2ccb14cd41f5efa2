"""One context walked across far-apart column STRUCTURES, and serving other entry points between two runs of a resident column.

tests/test_gpu_state_walk.py holds one resident column to a fresh one across far-apart states; here the context is what is held.  A
cs_ctx owns one Column whose device buffers never shrink (DevBuf::reserve keeps what is large enough), and workspace its entry points
share (the PHCO2 scratch, tmpA/B/C, the merged-table cache).  Each walk below sets column after column up on ONE context -- another
grid, level count, rule orders, absorber set, shape code, dispatch form and settings record per step, the larger structure before the
smaller one -- and at every step

  * builds the column on the walked context (it replaces the resident one), then on two fresh contexts under the same settings record;
  * holds sigma at the nodes, tau, M+, M- of the walked context to the fresh ones bitwise, and F+, F- bitwise where the two fresh
    columns agree bitwise, else at 5e-13 of the maximum (test_gpu_state_walk.same_as, unchanged);
  * runs the walked column a second time, and a third time after col.update to state B of test_gpu_state_walk.states() and back:
    both must reproduce the first run under the same rule (the re-run of a column that was set up over residue);
  * holds the step to the oracle at the state walk's tolerance for the absorber set (1e-11; 2e-11 with PHCO2; 1e-9 with pressure-
    shifted centres), every point up to 3000 points, the seeded 300-point sample above;
  * on a second visit to a structure, holds it to the first visit under the same rule;
  * asserts that what the step reports of its dispatch -- work()["dispatch"], info()["flux_form"], info()["line_kernel"] -- equals the
    fresh column's and differs from the previous step's: the walk crosses what it is meant to cross.

A step carries a complete settings record (SETTINGS_KEYS): the walked context keeps the previous step's settings, so every record is
applied in full, to the walked context and to the fresh ones.  tests/test_structure_walk_rules.py holds the step tables to the
conditions that keep the walks from being vacuous (no device needed).

What each walk is known to cover, by the sizes of its steps (cs_column_setup, sigma_impl, run_impl):
  voigt-forms     hot / cold / ranges (K x maxL, the hand-off words and per-(tile, state) flags), sigma, the near-line plane sigma2 (side
                  stream on and off), chebF with Kpad 32 -> 16 -> 32 -> 16 (padding states of a larger column under a smaller one), zones,
                  the interpolation levels on and off, the matrix-core piece tables
  flux-forms      ticket, partial and the group sums behind it, tau as k_flux_chunk's scratch, Mup / Mdn / F with 9 and 13 levels
  shape-codes     vvh (second code-5 group), ped (K = 12 then 9), PhScratch keyed by grid (both PHCO2 line kernels), the records of every code
  absorber-kinds  the column's tables, CIA pairs, knot cells, extra / S_toa / albedo switched on and off, the context's table and knot slots
  precision       the column's fp32 records (K x maxL, a longer table before a shorter one), fp64 after mixed
  interleaved     the PHCO2 scratch, tmpA/B/C, the line workspace of shape, bake and batch calls beside a resident (and captured) step

Measured on an MI355X (`pytest -s` prints the forms per step and the worst oracle errors).  Every comparison of the walked context with
a fresh one was bitwise, the band fluxes included (two fresh columns never differed), and so was every second visit, second run and
run after an update and back; every interleaved result equalled the fresh context's bitwise.  One residue was found, in the record only:
cs_column_work reported the 42 intervals of the previous column after a set-up with interpolation off (fixed: cs_column_setup clears the
count).  Worst error against the oracle over each walk, sigma / tau / M (of the column maximum) / F, and the time of the test:

  voigt-forms     1.2e-14 / 9.8e-15 / 2.7e-15 / 1.9e-15; forms 3 throughout, streams 1, 3, 1, 0, levels 4, 4, 3, 0; 0.7 s
  flux-forms      9.3e-15 / 7.1e-15 / 2.5e-15 / (sample); forms 2, 0 (k_rt_streams), 0, 3, 2; 0.7 s
  shape-codes     1.9e-14 / 1.4e-14 / 1.8e-13 / 2.9e-15; line kernels 0, 0, 0, 2, 1, 0, 0, 0, 0, groups 3, 2, 2, 2, 2, 2, 2, 2, 1; 0.9 s
  absorber-kinds  6.4e-14 / 5.3e-14 / 4.9e-15 / 2.1e-15 (the baked table: 6.4e-14); forms 0, 3, 0, 0, 3; 0.6 s
  precision       fp64 1.2e-14 / 8.6e-15 / 2.4e-12; mixed against fp64: sigma 3.6e-7 and 5.0e-7 (three tables), OLR 3.6e-8 and 2.8e-8 W/m^2; 0.5 s
  interleaved     11 launches and one near-line launch per run before and after every call, eager and replayed, fp64 and mixed; 0.3 - 0.6 s each
  PHCO2           24 launches with the levels laid out, 12 without; after the shape call 24, 12, 12 (eager and captured); 10 throughout with
                  interpolation off; 0.3 s each
"""
import numpy as np
import pytest

import tabulated_ref as R
import test_gpu_state_walk as SW
import workloads as W
from test_gpu_state_walk import MU, NU_A, NU_G, NU_L, NU_P, NU_S, states

pytestmark = pytest.mark.gpu


# ---- the settings record ------------------------------------------------------------------------------------------------------------------

TUNE_KEYS = (4, 7, 15)      # every tuning key a step of any walk touches: GRAPH, NEAR_STREAM, FLUX
SETTINGS_KEYS = ("precision", "far_s", "set_interp", "set_interp_plan", "set_matrix_cores", "set_merge", "tuning")


def settings(precision="fp64", far_s=1e6, interp=True, interp_plan=(-1, 128, 2048), matrix_cores=1, merge=True, tune=None):
    """a complete record, cs_create's defaults spelled out"""
    t = {4: 0, 7: 1, 15: 0}
    t.update(tune or {})
    assert set(t) == set(TUNE_KEYS)
    return dict(precision=precision, far_s=far_s, set_interp=interp, set_interp_plan=tuple(interp_plan), set_matrix_cores=matrix_cores,
                set_merge=merge, tuning=t)


def apply(ctx, rec):
    ctx.set_precision(rec["precision"], rec["far_s"])
    ctx.set_interp(rec["set_interp"])
    ctx.set_interp_plan(*rec["set_interp_plan"])
    ctx.set_matrix_cores(rec["set_matrix_cores"])
    ctx.set_merge(rec["set_merge"])
    for k in TUNE_KEYS:
        ctx.set_tuning(k, rec["tuning"][k])


class Step(SW.Spec):
    """one structure: the state walk's Spec (grid, levels, rule orders, members) under a complete settings record"""

    def __init__(self, label, nu, npl, members, rec, reference=SW.reference, **kw):
        super().__init__(nu, npl, members, **kw)
        self.label, self.settings, self.reference = label, rec, reference

    def context(self, cs):
        ctx = cs.Context(0)
        apply(ctx, self.settings)
        return ctx

    # what the rules count (Column: K = nl (nlobatto - 1) + 1)
    nnu = property(lambda self: len(self.nu))
    nl = property(lambda self: self.npl - 1)
    K = property(lambda self: (self.npl - 1) * (self.core[1] - 1) + 1)


def signature(r):
    """what a run reports of its dispatch"""
    return tuple(sorted(r["work"]["dispatch"].items())) + (("flux_form", r["info"]["flux_form"]), ("line_kernel", r["info"]["line_kernel"]))


def walk(cs, O, name, steps):
    """every step of `steps` on one context; returns the per-label first visits"""
    ctx = cs.Context(0)
    seen, prev, unmoved = {}, None, []
    try:
        for i, st in enumerate(steps):
            apply(ctx, st.settings)
            T = states(cs.pressuregrid(st.Pt, 1e5, st.npl), st.Tlim)
            col = st.column(cs, ctx, T["A"], MU["A"])
            assert ctx._resident is col
            r = SW.outputs(col)
            what = f"{name}: step {i} ({st.label})"
            if st.label not in seen:
                f1, f2 = SW.fresh(cs, st, T["A"], MU["A"]), SW.fresh(cs, st, T["A"], MU["A"])
                bitwise = bool(np.array_equal(f1["Fup"], f2["Fup"]) and np.array_equal(f1["Fdn"], f2["Fdn"]))
                for k in ("sigma", "tau", "Mup", "Mdn"):
                    assert np.array_equal(f1[k], f2[k]), (what, k, "two fresh columns differ")
                SW.same_as(r, f1, bitwise, what + " against a fresh column")
                worst = {}
                e = SW.vs_oracle(cs, O, st, col, r, worst, st.reference) if st.oracle else {}
                for k, v in e.items():
                    assert v < st.tol, (what, k, v)
                seen[st.label] = dict(r=r, fresh=f1, bitwise=bitwise, worst=worst)
                d = r["work"]["dispatch"]
                print(f"  {what}: K {col.K} x {col.nnu}, groups {r['info']['groups']}, form {r['info']['flux_form']}, line kernel "
                      f"{r['info']['line_kernel']}, far_split {d['far_split']} tables {d['tables']} streams {d['streams']} nodes_split "
                      f"{d['nodes_split']} flags {d['flags']}, levels {r['work']['levels']}, F bitwise {bitwise}, oracle "
                      + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
            else:
                print(f"  {what}: second visit")
            first = seen[st.label]
            f1 = first["fresh"]
            assert signature(r) == signature(f1) and r["info"] == f1["info"], (what, signature(r), signature(f1), r["info"], f1["info"])
            for k in r["work"]:      # every counter of the run, the near-line pairs the hand-off words carried among them
                assert k == "flux_scan_ns" or r["work"][k] == f1["work"][k], (what, k, r["work"][k], f1["work"][k])
            SW.same_as(r, first["r"], first["bitwise"], what + " against the first visit")
            SW.same_as(SW.outputs(col), first["r"], first["bitwise"], what + ", second run")
            col.update(T["B"], MU["B"])
            col.run()
            col.update(T["A"], MU["A"])
            SW.same_as(SW.outputs(col), first["r"], first["bitwise"], what + ", after an update to state B and back")
            assert ctx._resident is col
            if st.form is not None:
                assert r["info"]["flux_form"] == st.form, (what, r["info"])
            if st.check is not None:
                st.check(cs, st, r, first["fresh"])
            if signature(r) == prev:
                unmoved.append(what)
            prev = signature(r)
        worst = {}
        for v in seen.values():
            for k, e in v["worst"].items():
                worst[k] = max(worst.get(k, 0.0), e)
        print(f"  {name}: worst oracle error " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
        assert not unmoved, ("the reported dispatch did not change", unmoved)
        return seen
    finally:
        ctx.close()


# ---- voigt-forms ------------------------------------------------------------------------------------------------------------------------

def _ran_matrix_cores(cs, st, r, f):
    assert r["work"]["node_evals_matrix"] > 0 and r["work"]["direct_evals_matrix"] > 0, r["work"]


def _near_stream(on):
    def check(cs, st, r, f):
        assert bool(r["work"]["dispatch"]["streams"] & 2) == on, r["work"]["dispatch"]
    return check


def _no_levels(cs, st, r, f):
    assert r["work"]["levels"] == 0 and r["work"]["node_evals"] == 0, r["work"]


V_MX = Step("matrix cores 20000 x 21", 600.0 + 0.01 * np.arange(20000), 21, SW.synthetic(), settings(matrix_cores=2), check=_ran_matrix_cores)
V_SIDE = Step("NU_A x 9, near-line side stream", NU_A, 9, SW.fixtures(), settings(tune={7: 2}), check=_near_stream(True))
V_WHOLE = Step("NU_S x 9, three Lobatto nodes", NU_S, 9, SW.fixtures(), settings(), core=(4, 3), check=_near_stream(False))
V_OFF = Step("NU_A x 9, interpolation off", NU_A, 9, SW.fixtures(), settings(interp=False), check=_no_levels)
VOIGT_FORMS = [V_MX, V_SIDE, V_WHOLE, V_OFF, V_SIDE, V_MX]


def test_voigt_forms(cs, O):
    """a Voigt group throughout, K = 21, 9, 17, 9, 9, 21 (cheb_kpad 32, 16, 32, 16, 16, 32)"""
    walk(cs, O, "voigt-forms", VOIGT_FORMS)


# ---- flux-forms -------------------------------------------------------------------------------------------------------------------------

def _co2(cs, ctx, nu):
    return [cs.DirectGas(W.lines("fixture", "CO2"), SW.fC1, nu)]


def _rt_streams(on):
    def check(cs, st, r, f):
        assert bool(r["work"]["dispatch"]["flags"] & 4) == on, r["work"]["dispatch"]
    return check


def _flux_step(tiles, npl, tune, form, streams):
    return Step(f"{tiles} tiles x {npl}", np.linspace(640.0, 700.0, 64 * tiles), npl, _co2, settings(tune=tune), form=form, check=_rt_streams(streams))


# the state walk's configuration 7 (test_gpu_voigt_vvh.FORMS: grid size and key 15 pick the form), 9 and 13 levels in turn
F_4200, F_300, F_2000, F_600 = (_flux_step(4200, 9, {}, 2, False), _flux_step(300, 13, {15: 1}, 0, True), _flux_step(2000, 9, {}, 0, False),
                                _flux_step(600, 13, {}, 3, False))
FLUX_FORMS = [F_4200, F_300, F_2000, F_600, F_4200]


def test_flux_forms(cs, O):
    """k_flux_chunk (4200 tiles), k_rt_streams (300, key 15 = 1), k_rt (2000), k_flux_scan (600), k_flux_chunk again: ticket, partial,
    tau as scratch and the band partials of a longer grid under a shorter one, with more levels on the shorter grids"""
    walk(cs, O, "flux-forms", FLUX_FORMS)


# ---- shape-codes ------------------------------------------------------------------------------------------------------------------------

def _groups(n):
    def check(cs, st, r, f):
        assert r["info"]["groups"] == n, r["info"]
    return check


def _phco2_last(table):
    """test_gpu_state_walk.phco2's two gases with the PHCO2 gas last: info()["line_kernel"] is the last group's"""
    def members(cs, ctx, nu):
        return SW.phco2(table)(cs, ctx, nu)[::-1]
    return members


S_VVH2 = Step("code 5, two groups", NU_L, 9, SW.low("voigtVVH", second_cut=20.0), settings(), check=_groups(3))
S_CKD = Step("code 4 x 12, near-line side stream", NU_L, 12, SW.low("voigtCKD"), settings(tune={7: 2}), check=_near_stream(True))
S_CKDVVH = Step("code 6", NU_L, 9, SW.low("voigtCKDVVH"), settings())
S_PH_FAST = Step("PHCO2 dense (k_phco2)", NU_P, 9, _phco2_last("dense"), settings(), tol=2e-11)
S_PH_GEN = Step("PHCO2 fixture (k_linesum)", NU_G, 9, _phco2_last("fixture"), settings(), tol=2e-11)
S_LORENTZ = Step("lorentz", NU_A, 9, SW.fixtures("lorentz"), settings())
S_DOPPLER = Step("doppler, unfused flux", NU_A, 9, SW.fixtures("doppler"), settings(tune={15: 1}), form=0)
# arbitrary delta and P: 1e-9 (test_gpu_voigt_lbl's docstring: the device rounds nul + s, the restatement nu - s)
S_LBL = Step("code 7", NU_L, 9, SW.low("voigtLBL"), settings(), tol=1e-9)
S_VOIGT = Step("voigt, near-line side stream", NU_S, 9, SW.fixtures(), settings(tune={7: 2}), check=_near_stream(True))
SHAPE_CODES = [S_VVH2, S_CKD, S_CKDVVH, S_PH_FAST, S_PH_GEN, S_LORENTZ, S_DOPPLER, S_LBL, S_VOIGT, S_VVH2]


def test_shape_codes(cs, O):
    """one context through every shape code: the vvh plane of a second code-5 group, the pedestal workspace for 12 levels then 9, the
    PHCO2 scratch on two grids (both line kernels), codes 1, 2, 7 and 0, and the two code-5 groups again"""
    seen = walk(cs, O, "shape-codes", SHAPE_CODES)
    assert seen[S_PH_FAST.label]["r"]["info"]["line_kernel"] != seen[S_PH_GEN.label]["r"]["info"]["line_kernel"]


# ---- absorber-kinds ---------------------------------------------------------------------------------------------------------------------

def _gray_beam_extra(cs, ctx, nu):
    return SW.gray_beam(cs, ctx, nu) + [lambda v, T_, P_: 3e-27 * (P_ / 1e5) * (T_ / 250.0) * np.ones_like(v)]


KNOTS = 12


def _accelerated(cs, ctx, nu):
    Pk = cs.pressuregrid(10.0, 1e5, KNOTS)
    return [cs.AcceleratedAbsorber(states(Pk)["A"], Pk, *SW.fixtures()(cs, ctx, nu), ctx=ctx)]


def _accel_reference(cs, O, spec, col, idx):
    """the oracle's cross-sections at the knots, carried to the node pressures by tabulated_ref.accel_sigma (linear in ln P), as
    sigma_extra of an oracle column without gases"""
    A, x = col.accel, col.nu[idx]
    kc = A._knots
    kn = O.fluxes_discretized(x, A.P, 1.0, 2, kc.Tn, kc.mun, kc.Tlev, [g.sl for g in kc.gases], ["voigt"] * len(kc.gases),
                              [g.dnu_cut for g in kc.gases], kc.conc, nstream=1, want_sigma=True)
    L = np.log(kn["sigma"])
    extra = np.array([R.accel_sigma(L, A.P, p)[0] for p in col.Pk])
    r = O.fluxes_discretized(x, col.P, col.g, col.core.nlobatto, col.Tn, col.mun, col.Tlev, [], [], [], np.zeros((0, col.K)),
                             sigma_gray=col.sigma_gray, sigma_extra=extra, theta_s=col.theta_s, nstream=col.core.nstream, want_sigma=True)
    return r, r["sigma"]


def _nothing_left(cs, st, r, f):
    """a plain two-gas column after tables, pairs and knots: the fused flux form (a table would keep the separate kernels) and, as at
    every step, the launch count, launch groups and every work counter of a fresh column (a table, a pair or a knot slot left behind
    would add launches)"""
    assert r["info"] == f["info"] and r["info"]["flux_form"] != 0, (r["info"], f["info"])


A_BAKED = Step("baked beside direct", NU_A, 9, SW.baked, settings(), Tlim=(160.0, 480.0), form=0)
A_CIA = Step("CIA pairs", NU_A, 9, SW.cia_pairs, settings(), cia_data=SW._cia_sets())
A_GRAY = Step("gray + beam + albedo + sigma_extra, unfused flux", NU_S, 9, _gray_beam_extra, settings(tune={15: 1}),
              fS=lambda v: 2e-3 * np.exp(-((v - 670.0) / 20.0) ** 2), fa=0.3, form=0)
A_KNOTS = Step("accelerated knots", NU_S, 9, _accelerated, settings(), reference=_accel_reference, form=0)
A_PLAIN = Step("two gases", NU_A, 9, SW.fixtures(), settings(), check=_nothing_left)
ABSORBER_KINDS = [A_BAKED, A_CIA, A_GRAY, A_KNOTS, A_PLAIN, A_BAKED]


def test_absorber_kinds(cs, O):
    """a baked table beside a direct gas, CIA pairs, gray + beam + albedo with a host-evaluated term, an accelerated absorber (whose knot
    column replaces the resident one before the flux column does), a plain two-gas column that must show nothing of them, the table again"""
    walk(cs, O, "absorber-kinds", ABSORBER_KINDS)


# ---- precision --------------------------------------------------------------------------------------------------------------------------

NU_M = np.linspace(600.0, 760.0, 4000)       # test_gpu_state_walk.test_mixed_precision's grid


def _three(cs, ctx, nu):
    return SW.fixtures()(cs, ctx, nu) + [cs.DirectGas(W.lines("fixture", "CH4"), SW.fC2, nu)]


def _against_fp64(cs, st, r, f):
    """test_mixed_precision_variant's bounds: cross-sections within 1e-6 of the fp64 path, OLR within 1e-5 W/m^2 (and the fp32 bodies ran)"""
    ref = Step("fp64", st.nu, st.npl, st.members, settings(tune=st.settings["tuning"]), core=st.core)
    T = states(cs.pressuregrid(st.Pt, 1e5, st.npl), st.Tlim)
    d = SW.fresh(cs, ref, T["A"], MU["A"])
    m = d["sigma"] > 0
    e = float(np.max(np.abs(r["sigma"][m] / d["sigma"][m] - 1.0)))
    print(f"  {st.label}: sigma against fp64 {e:.1e}, OLR {abs(r['Fup'][0] - d['Fup'][0]):.1e} W/m^2")
    assert 0.0 < e < 1e-6 and abs(r["Fup"][0] - d["Fup"][0]) < 1e-5, (st.label, e)


P_64 = Step("fp64", NU_M, 21, SW.fixtures(), settings(), check=_near_stream(False))
P_MIXED = Step("mixed, near-line side stream", NU_M, 21, SW.fixtures(), settings(precision="mixed", tune={7: 2}), oracle=False, check=_against_fp64)
P_LONG = Step("mixed, three tables on 6000 points, unfused flux", np.linspace(600.0, 760.0, 6000), 21, _three,
              settings(precision="mixed", tune={7: 2, 15: 1}), oracle=False, form=0, check=_against_fp64)
PRECISION = [P_64, P_MIXED, P_64, P_LONG, P_MIXED, P_64]


def test_precision(cs, O):
    """fp64, mixed (far_s = 1e6), fp64 on one structure, mixed on a longer table and grid, then the first two again: the fp32 records of a
    longer table under a shorter one; fp64 after mixed is the fresh fp64 bitwise (and the first visit)"""
    seen = walk(cs, O, "precision", PRECISION)
    assert not np.array_equal(seen[P_64.label]["r"]["sigma"], seen[P_MIXED.label]["r"]["sigma"])


# ---- interleaved calls ------------------------------------------------------------------------------------------------------------------

# the resident column, and what the context serves between its runs: a shape call on a longer table at more states than the column has
# (K L > K maxL: a context-owned fp32 workspace would be reallocated), a batch of B profiles (B K > K)
I_COLUMN = Step("resident", NU_A, 9, SW.fixtures(), settings())
I_SHAPE_TABLE, I_SHAPE_STATES, I_BATCH = ("synthetic", "CO2"), 30, 3
I_PH_COLUMN = Step("resident PHCO2", NU_P, 9, _phco2_last("dense"), settings())
I_PH_STATES = 20


def _shape_states(n):
    x = np.linspace(0.0, 1.0, n)
    P = 10.0 * (1e5 / 10.0) ** x
    return 180.0 + 140.0 * x, P, 4e-4 * P


def _knots(cs, ctx):
    """the accelerated absorber of the interleaved calls: built before the resident column, whose setup replaces its knot column"""
    Pk = cs.pressuregrid(10.0, 1e5, KNOTS)
    return cs.AcceleratedAbsorber(states(Pk)["A"], Pk, *SW.fixtures()(cs, ctx, NU_S), ctx=ctx)


def _calls(cs, ctx, col, A):
    """(name, call) in the order the context serves them between two runs of `col`; each call returns a tuple of arrays"""
    nu_b = 600.0 + 0.01 * np.arange(2000)
    T, P, Pp = _shape_states(I_SHAPE_STATES)
    Tl = states(col.P)
    x = np.linspace(-30.0, 30.0, 4001)

    def bake():
        Om = cs.AtmosphericDomain(SW.DOMAIN, 5, (5.0, 2e5), 6)
        g = cs.Gas(W.lines("fixture", "CO2"), 4e-4, NU_S, Om, ctx=ctx, keep_host_tables=True)
        return g.lnsigma, g.rawsigma(251.3, 3.1e4)
    return [("shape_batch", lambda: (cs.shape_batch(W.lines(*I_SHAPE_TABLE), "voigt", nu_b, T, P, Pp, 25.0, ctx),)),
            ("shape_points", lambda: (cs.shape_points(W.lines("fixture", "H2O"), "voigt", nu_b[::7], T[:5], P[:5], Pp[:5], 25.0, ctx),)),
            ("bake and rawsigma", bake),
            ("Sigma of an accelerated absorber", lambda: (np.array([cs.Sigma(A, 1500, 250.0, 3.1e4)]), A(3.1e4))),
            ("faddeeva", lambda: (cs.faddeeva(x, np.abs(x) * 1e-3 + 1e-6, ctx),)),
            ("run_batch", lambda: col.run_batch([Tl[s] for s in "ABC"[:I_BATCH]], [MU[s] for s in "ABC"[:I_BATCH]]))]


def _resident(cs, st, ctx):
    T = states(cs.pressuregrid(st.Pt, 1e5, st.npl), st.Tlim)
    col = st.column(cs, ctx, T["A"], MU["A"])
    setups, inner = [0], col._setup

    def counted():
        setups[0] += 1
        inner()
    col._setup = counted
    return col, setups, T


def _fresh_pair(cs, st, T):
    f1, f2 = SW.fresh(cs, st, T["A"], MU["A"]), SW.fresh(cs, st, T["A"], MU["A"])
    return f1, bool(np.array_equal(f1["Fup"], f2["Fup"]) and np.array_equal(f1["Fdn"], f2["Fdn"]))


def _on_fresh_context(cs, st, T, name):
    """the interleaved call `name` on a context of its own, set up like the walked one"""
    c2 = st.context(cs)
    try:
        A2 = _knots(cs, c2)
        col2 = st.column(cs, c2, T["A"], MU["A"])
        want = dict(_calls(cs, c2, col2, A2))[name]()
        del col2, A2
        return want
    finally:
        c2.close()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_interleaved_calls(cs, precision, graph):
    """one resident column on NU_A (near-line kernels on their side stream); between its runs the context serves cs_shape_batch (a longer
    table, more states), cs_shape_points, cs_bake + cs_table_eval, cs_accel_eval, cs_faddeeva_batch and cs_column_batch (B = 3).  After
    each the column's next run reproduces its first outputs bitwise without a new setup, and each interleaved result equals the same call
    on a fresh context bitwise.  With key 4 the step has been captured and replayed before the first interleaved call: every later run
    reports the captured run's launch count, near-line launches and dispatch (test_graph_replay_keeps_near_plane_bookkeeping's facts:
    launches > 0 and the cross-sections with the near-line plane folded in, here bitwise).  mixed + graph: a captured step names fp32
    records, which are the column's own -- a shape, bake or batch call brings its own and cannot move them"""
    st = Step(I_COLUMN.label, I_COLUMN.nu, I_COLUMN.npl, I_COLUMN.members, settings(precision=precision, tune={4: int(graph), 7: 2}))
    ctx = st.context(cs)
    try:
        A = _knots(cs, ctx)
        col, setups, T = _resident(cs, st, ctx)
        f1, bitwise = _fresh_pair(cs, st, T)
        runs = [SW.outputs(col) for _ in range(3)]          # under key 4: eager, captured, replayed
        for n, r in enumerate(runs):
            SW.same_as(r, f1, bitwise, f"run {n} against a fresh column")
        base, book = runs[0], runs[2]
        assert base["work"]["dispatch"]["streams"] & 2 and base["info"]["launches"] > 0, (base["work"]["dispatch"], base["info"])
        for name, call in _calls(cs, ctx, col, A):
            got, want = call(), _on_fresh_context(cs, st, T, name)
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert np.array_equal(a, b), (name, float(np.nanmax(np.abs(np.asarray(a) - np.asarray(b)))))
            r = SW.outputs(col)
            SW.same_as(r, base, bitwise, f"the run after {name}")
            assert setups[0] == 0 and ctx._resident is col, (name, setups[0])
            assert r["info"] == book["info"] and r["work"]["dispatch"] == book["work"]["dispatch"], (name, r["info"], book["info"],
                                                                                                     r["work"]["dispatch"], book["work"]["dispatch"])
            print(f"  {precision} {'graph' if graph else 'eager'}: after {name}: launches {r['info']['launches']}, near-line launches "
                  f"{r['info']['near_launches']}, dispatch {r['work']['dispatch']}")
        del A
    finally:
        ctx.close()


@pytest.mark.parametrize("graph,interp", [(False, True), (True, True), (True, False)], ids=["eager", "graph", "graph-interp-off"])
def test_interleaved_phco2(cs, graph, interp):
    """a resident PHCO2 column (k_phco2) with one cs_shape_batch of PHCO2 on another grid and at more states in between: the call resets
    the grid of the context's PHCO2 scratch and moves its per-(state, line) factors, so the column's next run lays the levels out again
    (interpolation on) or runs on moved buffers (off) -- a captured step is dropped for either -- and reproduces the first outputs bitwise"""
    st = Step(I_PH_COLUMN.label, I_PH_COLUMN.nu, I_PH_COLUMN.npl, I_PH_COLUMN.members, settings(interp=interp, tune={4: int(graph)}), tol=2e-11)
    ctx = st.context(cs)
    try:
        col, setups, T = _resident(cs, st, ctx)
        f1, bitwise = _fresh_pair(cs, st, T)
        runs = [SW.outputs(col) for _ in range(3)]
        for n, r in enumerate(runs):
            SW.same_as(r, f1, bitwise, f"run {n} against a fresh column")
        assert runs[0]["info"]["line_kernel"] == 2, runs[0]["info"]
        first, steady = runs[0]["info"]["launches"], runs[2]["info"]["launches"]
        assert 0 < steady <= first and runs[1]["info"]["launches"] == steady, (first, steady)
        Ts, Ps, Pp = _shape_states(I_PH_STATES)

        def call(c):
            return cs.shape_batch(SW.dense(cs), "PHCO2", NU_P + 60.0, Ts, Ps, Pp, 500.0, c)
        got = call(ctx)
        c2 = st.context(cs)
        try:
            assert np.array_equal(got, call(c2))
        finally:
            c2.close()
        after = [SW.outputs(col) for _ in range(3)]
        for n, r in enumerate(after):
            SW.same_as(r, runs[0], bitwise, f"run {n} after the PHCO2 shape call")
        assert setups[0] == 0 and ctx._resident is col
        assert after[0]["info"]["launches"] in (first, steady) and after[1]["info"]["launches"] == steady and after[2]["info"] == runs[2]["info"]
        print(f"  PHCO2 {'graph' if graph else 'eager'}, interpolation {interp}: launches {first} then {steady}; after the shape call "
              f"{[r['info']['launches'] for r in after]}")
    finally:
        ctx.close()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_other_bands_under_a_resident_cia_column_are_refused(cs, lines, graph):
    """a resident column's CIA pairs hold the addresses of the slot's band tables; cs_cia_begin / cs_cia_band / cs_cia_clear free those.
    The next run (eager, or the replay of a captured step) and the next batch are refused (CS_ESTATE) until cs_column_set_cia is called
    again, after which the same bands give the first result bitwise.  Read from the code, like the slots of gases, tables and knots"""
    import test_gpu_cia_bands as CB
    nu = R.grid(160)
    data = R.overlap_set(2)
    ctx = cs.Context(0)
    try:
        apply(ctx, settings(tune={4: int(graph)}))
        CB._upload(cs, ctx, 0, data)
        col = CB._bare_column(cs, lines, ctx, nu, 10, 3)
        P1, P2 = 0.6 * col.Pk[None, :], 0.3 * col.Pk[None, :]
        CB._set_cia(cs, ctx, [0], P1, P2)
        runs = [SW.outputs(col) for _ in range(3)]
        for r in runs[1:]:
            SW.same_as(r, runs[0], True, "the column before the slot changes")
        for change in ("refilled", "cleared"):
            if change == "refilled":
                CB._upload(cs, ctx, 0, data)
            else:
                cs.check(cs.lib().cs_cia_clear(ctx.handle, 0))
            for call in (col.run, lambda: col.run_batch([col.Tlev, col.Tlev + 1.0])):
                with pytest.raises(cs.ClearSkyHIPError) as ei:
                    call()
                assert ei.value.code == -6 and "CIA slot 0" in str(ei.value), (change, str(ei.value))
            if change == "cleared":
                CB._upload(cs, ctx, 0, data)
            CB._set_cia(cs, ctx, [0], P1, P2)
            for n in range(3):
                SW.same_as(SW.outputs(col), runs[0], True, f"run {n} after the slot was {change} and the pairs were set again")
    finally:
        ctx.close()
