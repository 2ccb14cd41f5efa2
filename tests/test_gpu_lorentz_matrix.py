"""The Lorentz shape (code 1) with its far wings and window ends on the matrix cores: k_cheb_nodes_mx<true>, k_voigt_edge_mx<SPLIT, true>
and k_voigt_far<false, S, true, true> behind the plan of voigt_plan (tests/test_lorentz_series.py states the series they sum).

Forms, run_column and the crowd cases are test_gpu_isolated_line's, test_gpu_crowded_lines' and crowded_line_ref's; the walk states, the
members and the oracle comparison test_gpu_state_walk's; the piece-table forms test_gpu_dispatch's; the chunk rule test_gpu_state_chunks'.

  a  piece thresholds     M copies of one line on both sides of 8, 16 and 48 as shape `lorentz` under eight forms against 40 digits (the hard
                          bound of code 1); the matrix counters 0 at M = 7 and positive at M = 8; no 8-term, sub-tile or near-line work ever
  b  matrix | vector      cs_shape_batch and cs_shape_points of the CO2 and H2O fixtures, K = 1, 15, 16, 17, 33, cut-offs 1, 5, 25: the matrix
                          cores forced against the vector unit (5e-13 of the maximum) and the oracle (5e-12); the 20 000 x 21 column under
                          the default dispatch, which must report matrix work
  c  table, kernel forms  the three piece-table forms: equal tables (work counts) and bitwise columns; four waves per item and one item per
                          wave in both kernels, far pieces on 16 / 32 / 64 nodes (keys 11, 17), ends at the points (key 23): oracle at 1e-11
  d  columns              alone, two merged Lorentz gases, Voigt beside Lorentz, Lorentz beside a baked table, CIA pairs and the gray term;
                          every flux form; run_batch of three states, an accelerated absorber, a baked 4 x 4 domain, two nu-shards
  e  state chunks         cs_shape_batch in three chunks or more with a ragged last group, bitwise the same states called chunk by chunk
  f  what must not move   code 1 | CS_SHAPE_PSHIFT and matrix-cores-0 report no matrix work; a resident column walked A B C A, eager and
                          captured, is bitwise a fresh one; work()["dispatch"] is the plan that ran; two runs are bitwise equal

Recorded figures (MI355X): see profiles/lorentz_matrix_cores.md.  Worst error / hard bound over the forms of a: see there.
"""
import numpy as np
import pytest

import clearsky_jl_amd
import crowded_line_ref as X
import isolated_line_ref as I
import test_gpu_crowded_lines as TC
import test_gpu_dispatch as D
import test_gpu_isolated_line as T
import test_gpu_state_chunks as CH
import test_gpu_state_walk as SW
import workloads as W
from conftest import relerr

pytestmark = pytest.mark.gpu

MATRIX = ("node_evals_matrix", "direct_evals_matrix", "matrix_evals_3term")
NEVER = ("matrix_evals_8term", "sub_evals", "near_pairs_tier0", "near_pairs_tier1", "core_tile_states")


def _no_voigt_work(w, info, what):
    assert all(w[c] == 0 for c in NEVER), (what, {c: w[c] for c in NEVER})
    assert info["near_launches"] == 0, (what, info)


def _matrix_work(w):
    return {c: w[c] for c in MATRIX}


# ---- a. piece thresholds ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def crowd(cs):
    cases = X.Cases(cs)
    made = {}

    def get(groups, name):
        if name not in made:
            made[name] = X.CrowdCase(cs, name, cases.short, cases.plan(cases.short), [groups], cases.column(), code=1)
        return made[name]
    get.mid, get.next = cases.mid, float(cases.short[20 * 64 + 33])
    return get


def _lorentz_forms(cs, case):
    """every form of test_gpu_crowded_lines.FORMS_A on one Lorentz crowd: {form: (worst / hard bound, work, info)}"""
    case.reference()
    rows = {}
    for f in TC.FORMS_A:
        r = T.run_column(cs, case, f, "lorentz")
        hard, _ = X.compare(case, r["got"], f.model(len(case.sizes)), f"{case.name} {f.name}")
        _no_voigt_work(r["work"], r["info"], f"{case.name} {f.name}")
        rows[f.name] = (hard, r["work"], r["info"])
        print(f"{case.name} {f.name}: worst error / hard bound {hard:.3f}, matrix work {_matrix_work(r['work'])}")
    return rows


@pytest.mark.parametrize("M", X.M_THRESHOLDS)
def test_piece_thresholds(cs, crowd, M):
    """M copies at col/short-cluster's centre, shape lorentz, eight forms, the hard bound of code 1 at every probe.  With the matrix
    cores forced the vector unit keeps every piece at M = 7 and the matrix cores sum node pieces, window pieces and 3-term parts from
    M = 8 on (what fails before the Lorentz pieces existed: all three counters were 0 at every M)"""
    rows = _lorentz_forms(cs, crowd([(crowd.mid, M, 1.0)], f"lor/M{M}"))
    w = rows["matrix-cores-2"][1]
    if M >= 8:
        assert all(w[c] > 0 for c in MATRIX), _matrix_work(w)
    else:
        assert all(w[c] == 0 for c in MATRIX), _matrix_work(w)
    w0 = rows["matrix-cores-0"][1]
    assert all(w0[c] == 0 for c in MATRIX) and w0["dispatch"]["tables"] == 0, w0


@pytest.mark.parametrize("split", X.SPLITS, ids=[f"{a}+{b}" for a, b in X.SPLITS])
def test_split_clusters(cs, crowd, split):
    """a + b copies one grid step apart: a piece counts the lines of its zone, whatever their centres"""
    a, b = split
    rows = _lorentz_forms(cs, crowd([(crowd.mid, a, 1.0), (crowd.next, b, 1.0)], f"lor/split-{a}+{b}"))
    w = rows["matrix-cores-2"][1]
    assert all(w[c] > 0 for c in MATRIX), _matrix_work(w)


# ---- b. matrix against vector, and against the oracle ------------------------------------------------------------------------------------------

K_B = (1, 15, 16, 17, 33)
NU_B = {"CO2": np.linspace(640.0, 700.0, 6000), "H2O": np.linspace(1500.0, 1560.0, 6000)}


def _ctx(cs, mc, tune=()):
    ctx = cs.Context(0)
    ctx.set_matrix_cores(mc)
    for k, v in tune:
        ctx.set_tuning(k, v)
    return ctx


def _close_max(a, b, tol=5e-13, rows=True):
    """device against device at the suite's 5e-13 of the maximum: of each row (a state's cross-sections), or of the whole array (fluxes)"""
    scale = np.max(np.abs(b), axis=-1, keepdims=True) if rows else np.max(np.abs(b))
    assert np.all(np.isfinite(a)) and np.all(scale > 0)
    e = float(np.max(np.abs(a - b) / scale))
    assert e < tol, e
    return e


@pytest.mark.parametrize("K", K_B)
@pytest.mark.parametrize("gas", ["CO2", "H2O"])
def test_batch_and_points_matrix_against_vector(cs, O, lines, gas, K):
    """the padded lanes of the last state group (K = 1, 15, 17), whole groups (16) and three groups (33): matrix-cores-2 against
    matrix-cores-0 at 5e-13 of the row's maximum and against the oracle at 5e-12 (test_lorentz_fast_path's bar), cut-offs 1, 5, 25"""
    sl, nu = lines(gas), NU_B[gas]
    Tk, P, Pp = (np.array(x) for x in zip(*I.batch_states(K)))
    on, off = _ctx(cs, 2), _ctx(cs, 0)
    try:
        for cut in (1.0, 5.0, 25.0):
            for fn, strict in ((cs.shape_batch, True), (cs.shape_points, False)):
                a = fn(sl, "lorentz", nu, Tk, P, Pp, cut, on)
                b = fn(sl, "lorentz", nu, Tk, P, Pp, cut, off)
                e = _close_max(a, b)
                worst = 0.0
                for k in sorted({0, K // 2, K - 1}):
                    so = O.shape_bang("lorentz", nu, sl, Tk[k], P[k], Pp[k], cut, strict_ends=strict)
                    assert np.array_equal(a[k] == 0, so == 0)
                    worst = max(worst, relerr(a[k], so, floor=1e-250))
                assert worst < 5e-12, (fn.__name__, cut, worst)
                print(f"{gas} K = {K} cut {cut} {fn.__name__}: matrix | vector {e:.1e} of the maximum, oracle {worst:.1e}")
    finally:
        on.close()
        off.close()


def _lorentz_synthetic(cs, ctx, nu):
    return [cs.DirectGas(W.lines("synthetic", "CO2"), SW.fC1, nu, shape="lorentz"), cs.DirectGas(W.lines("synthetic", "H2O"), SW.fC2, nu, shape="lorentz")]


NU_MX = 600.0 + 0.01 * np.arange(20000)          # test_gpu_state_walk's "matrix cores" column: 20 000 points, 21 levels


def test_default_dispatch_reports_matrix_work(cs, O):
    """the 20 000 x 21 column under the DEFAULT dispatch: the Lorentz group's node sums and window pieces run on the matrix cores; against
    matrix-cores-0 at 5e-13 of the maximum and against the oracle on the sample at 1e-11"""
    Tl = SW.states(cs.pressuregrid(10.0, 1e5, 21))["A"]
    spec = SW.Spec(NU_MX, 21, _lorentz_synthetic)
    off = SW.Spec(NU_MX, 21, _lorentz_synthetic, setup=lambda ctx: ctx.set_matrix_cores(0))
    a, b = SW.fresh(cs, spec, Tl, SW.MU["A"]), SW.fresh(cs, off, Tl, SW.MU["A"])
    assert all(a["work"][c] > 0 for c in MATRIX) and a["work"]["dispatch"]["tables"] != 0, (_matrix_work(a["work"]), a["work"]["dispatch"])
    assert all(b["work"][c] == 0 for c in MATRIX) and b["work"]["dispatch"]["tables"] == 0, _matrix_work(b["work"])
    assert a["info"]["groups"] == 1
    _no_voigt_work(a["work"], a["info"], "default")
    for k in ("sigma", "tau", "Mup", "Mdn"):
        _close_max(a[k], b[k], rows=k in ("sigma", "tau"))
    ctx = spec.context(cs)
    try:
        col = spec.column(cs, ctx, Tl, SW.MU["A"])
        r = SW.outputs(col)
        worst = {}
        SW.vs_oracle(cs, O, spec, col, r, worst)
        for k in ("sigma", "tau", "Mup", "Mdn"):
            assert np.array_equal(r[k], a[k]), k
    finally:
        ctx.close()
    print("default dispatch:", _matrix_work(a["work"]), a["work"]["dispatch"], "oracle", worst)
    assert all(v < 1e-11 for v in worst.values()), worst


# ---- c. every table form and kernel form ------------------------------------------------------------------------------------------------------

def _run_lorentz(n, np_=17, tune=(), mc=2, p_surf=1e5):
    """test_gpu_dispatch._run with both synthetic gases as shape lorentz"""
    cs = clearsky_jl_amd
    nu = D._nu(n)
    P = cs.pressuregrid(10.0, p_surf, np_)
    Tl = W.earth_temperature(P)
    ctx = _ctx(cs, mc, tune)
    try:
        col = cs.Column(P, 9.8, Tl, 0.029, 0.0, 0.0, *_lorentz_synthetic(cs, ctx, nu), core=cs.Discretized(5, 2), ctx=ctx)
        r = SW.outputs(col)
        r["col"], r["nu"] = col, nu
    finally:
        ctx.close()
    return r


def _oracle_column(O, r, tol=1e-11):
    col, n = r["col"], len(r["nu"])
    idx = SW.sample(n)
    ref = O.fluxes_discretized(col.nu[idx], col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [g.sl for g in col.gases], [g.shape for g in col.gases],
                               [g.dnu_cut for g in col.gases], col.conc, want_sigma=True)
    sm = max(ref["Mup"].max(), ref["Mdn"].max())
    e = dict(sigma=relerr(r["sigma"][:, idx], ref["sigma"], floor=1e-280), tau=relerr(r["tau"][:, idx], ref["tau"]),
             Mup=float(np.max(np.abs(r["Mup"][:, idx] - ref["Mup"])) / sm), Mdn=float(np.max(np.abs(r["Mdn"][:, idx] - ref["Mdn"])) / sm))
    assert all(v < tol for v in e.values()), e
    return e


@pytest.mark.parametrize("np_,p_surf,tiles", [(17, 5e3, 40), (40, 1e5, 135)], ids=["K17", "K40"])
def test_piece_table_forms_same_tables(O, np_, p_surf, tiles):
    """the piece tables of a Lorentz group as blocks of k_gas_setup_mx, by k_mxzones16 and by k_mxzones (test_gpu_dispatch.TABLE_FORMS),
    a last tile of ONE point, a second state group of one state (K = 17, levels up to 5e3 Pa: lines narrow enough for the 3-term split) or half filled (K = 40): equal work counts -- cs_column_work
    counts from the tables it reads back -- and bitwise equal columns; none of them holds a core"""
    n = 64 * (tiles - 1) + 1
    runs = [_run_lorentz(n, np_, ((1, 1),) + tune, p_surf=p_surf) for tune, _ in D.TABLE_FORMS]
    for r, (tune, form) in zip(runs, D.TABLE_FORMS):
        assert r["work"]["dispatch"]["tables"] == form, (tune, r["work"]["dispatch"])
        _no_voigt_work(r["work"], r["info"], tune)
    for r in runs[1:]:
        for k in ("sigma", "tau", "Mup", "Mdn", "Fup", "Fdn"):
            assert np.array_equal(r[k], runs[0][k]), k
        assert D._work_but_form(r) == D._work_but_form(runs[0])
    w = runs[0]["work"]
    assert all(w[c] > 0 for c in MATRIX[:2 if np_ == 40 else 3]), _matrix_work(w)      # (up to 1e5 Pa a group's widest state leaves no 3-term part)
    print(f"K = {np_}, {tiles} tiles:", _matrix_work(w), _oracle_column(O, runs[0]))


# (tiles, levels, tuning): four waves per item in both kernels (short grid), one item per wave (1441 tiles x 3 groups: mx_big), the far
# pieces on all 64 nodes (key 11), on 64 because every item is shared (key 17), the window ends at the points (key 23)
KERNEL_FORMS = [("four-waves-per-item", 135, 17, ()), ("one-item-per-wave", 1441, 34, ()), ("far-pieces-64", 1441, 34, ((11, 1),)),
                ("far64-shared", 135, 17, ((17, 1),)), ("ends-at-points", 1441, 34, ((23, 1),))]


@pytest.mark.parametrize("name,tiles,np_,tune", KERNEL_FORMS, ids=[f[0] for f in KERNEL_FORMS])
def test_kernel_forms_against_oracle(O, name, tiles, np_, tune):
    r = _run_lorentz(64 * tiles, np_, tune)
    w, d = r["work"], r["work"]["dispatch"]
    assert all(w[c] > 0 for c in MATRIX[:2]), (name, _matrix_work(w))
    _no_voigt_work(w, r["info"], name)
    flags = clearsky_jl_amd.DISPATCH_FLAGS
    if name == "one-item-per-wave":
        assert d["flags"] & flags["TNODES"] and d["nodes_split"] == 0, d
    if name == "ends-at-points":
        assert not d["flags"] & flags["TNODES"], d
    if name == "far64-shared":
        assert d["flags"] & flags["FAR64_SHARED"], d
    if name == "four-waves-per-item":
        assert not d["flags"] & flags["TNODES"] and not d["flags"] & flags["FAR64_SHARED"], d
    print(name, _matrix_work(w), d, _oracle_column(O, r))


# ---- d. columns ------------------------------------------------------------------------------------------------------------------------------------

def _alone(cs, ctx, nu):
    return [cs.DirectGas(W.lines("fixture", "CO2"), SW.fC1, nu, shape="lorentz")]


def _voigt_beside(cs, ctx, nu):
    return [cs.DirectGas(W.lines("fixture", "CO2"), SW.fC1, nu), cs.DirectGas(W.lines("fixture", "H2O"), SW.fC2, nu, shape="lorentz")]


def _with_members(cs, ctx, nu):
    d = SW._cia_sets()
    Om = cs.AtmosphericDomain(SW.DOMAIN, 8, (5.0, 2e5), 10)
    g = cs.Gas(W.lines("fixture", "H2O"), lambda T, P: min(0.3, 1e-3 * (P / 1e5) * (T / 250.0) ** 4), nu, Om, ctx=ctx, keep_host_tables=True)
    return [cs.DirectGas(W.lines("fixture", "CO2"), SW.fC1, nu, shape="lorentz"), g, cs.CIATables(d["CO2-CO2"], extrapolate=True), cs.GrayGas(2e-26, nu)]


COLUMNS = {"alone": (_alone, 1, {}), "merged": (SW.fixtures("lorentz", "lorentz"), 1, {}), "voigt-beside": (_voigt_beside, 2, {}),
           "members": (_with_members, 1, dict(Tlim=(160.0, 480.0), cia_data=SW._cia_sets()))}


@pytest.mark.parametrize("tiles,tune,form,streams", SW._forms(), ids=[f"{t}tiles-{f}{'-streams' if s else ''}{'-unfused' if u else ''}" for t, u, f, s in SW._forms()])
@pytest.mark.parametrize("name", list(COLUMNS))
def test_columns_every_flux_form(cs, O, name, tiles, tune, form, streams):
    """sigma, tau to 1e-11 and M, F to 1e-11 of the column maximum against the oracle under the scan form, k_rt, k_rt_streams and the chunk
    form, the matrix cores forced; every Voigt / Lorentz group of the column with matrix work (one Lorentz group: no near-line launch)"""
    members, groups, kw = COLUMNS[name]
    spec = SW.Spec(np.linspace(640.0, 700.0, 64 * tiles), 9, members, tune=tuple(tune.items()), setup=SW.matrix_cores, **kw)
    Tl = SW.states(cs.pressuregrid(spec.Pt, 1e5, spec.npl), spec.Tlim)["A"]
    ctx = spec.context(cs)
    try:
        col = spec.column(cs, ctx, Tl, SW.MU["A"])
        r = SW.outputs(col)
        want = 0 if name == "members" else form      # (flux_plan: a column with a baked table keeps k_rt / k_rt_streams on every grid)
        assert r["info"]["flux_form"] == want and r["info"]["groups"] == groups, r["info"]
        assert bool(r["work"]["dispatch"]["flags"] & 4) == streams
        assert r["work"]["node_evals_matrix"] > 0, _matrix_work(r["work"])      # (the fixtures' window ends are shorter than 8 lines: node pieces only)
        if name != "voigt-beside":
            _no_voigt_work(r["work"], r["info"], name)
        worst = {}
        SW.vs_oracle(cs, O, spec, col, r, worst)
        again = SW.outputs(col)
        for k in ("sigma", "tau", "Mup", "Mdn"):
            assert np.array_equal(again[k], r[k]), k
    finally:
        ctx.close()
    print(name, tiles, form, _matrix_work(r["work"]), worst)
    assert all(v < 1e-11 for v in worst.values()), worst


def test_batch_of_three_states(cs):
    """cs_column_batch of three states against three sequential updates (5e-13 of the largest flux)"""
    spec = SW.Spec(SW.NU_A, 9, SW.fixtures("lorentz", "lorentz"), setup=SW.matrix_cores)
    Ts = SW.states(cs.pressuregrid(spec.Pt, 1e5, spec.npl))
    ctx = spec.context(cs)
    try:
        col = spec.column(cs, ctx, Ts["A"], SW.MU["A"])
        seq = []
        for s in "ABC":
            col.update(Ts[s])
            r = SW.outputs(col)
            assert r["work"]["node_evals_matrix"] > 0
            seq.append((r["Fup"].copy(), r["Fdn"].copy()))
        Fup, Fdn = col.run_batch([Ts[s] for s in "ABC"])
        for b in range(3):
            fm = max(np.abs(seq[b][0]).max(), np.abs(seq[b][1]).max())
            assert np.max(np.abs(Fup[b] - seq[b][0])) < 5e-13 * fm and np.max(np.abs(Fdn[b] - seq[b][1])) < 5e-13 * fm, b
    finally:
        ctx.close()


def test_accelerated_absorber_and_bake(cs, O, lines):
    """cs_accel_store and cs_bake of a 4 x 4 domain go through line_sum_voigt: matrix-cores-2 against matrix-cores-0 at 5e-13 of the
    maximum, and the baked knots against the oracle at 5e-12"""
    sl, nu = lines("CO2"), NU_B["CO2"]
    Pk = np.geomspace(10.0, 1e5, 12)
    Tk = np.linspace(200.0, 290.0, 12)
    out = {}
    for mc in (2, 0):
        ctx = _ctx(cs, mc)
        try:
            A = cs.AcceleratedAbsorber(Tk, Pk, cs.DirectGas(sl, 400e-6, nu, shape="lorentz"), ctx=ctx)
            dom = cs.AtmosphericDomain((200.0, 320.0), 4, (10.0, 1e5), 4)
            g = cs.Gas(sl, 400e-6, nu, dom, shape="lorentz", ctx=ctx)
            out[mc] = (A(float(Pk[3])), np.array([[g.rawsigma(T, P) for P in dom.P] for T in dom.T]), dom)
        finally:
            ctx.close()
    assert np.max(out[0][0]) > 0
    _close_max(out[2][0], out[0][0])
    a, b, dom = out[2][1], out[0][1], out[2][2]
    _close_max(a, b)
    for ti, ki in ((0, 0), (3, 3), (1, 2)):
        so = O.shape_bang("lorentz", nu, sl, dom.T[ti], dom.P[ki], 400e-6 * dom.P[ki], 25.0)
        assert relerr(a[ti, ki], so, floor=1e-250) < 5e-12, (ti, ki)


def test_two_shards_add_up(cs):
    """two nu-shards of one grid: their band fluxes add up to the whole column's (5e-13), each shard with matrix work of its own"""
    nu = NU_MX[:12800]
    P = cs.pressuregrid(10.0, 1e5, 17)
    Tl = W.earth_temperature(P)
    F = []
    for rng in (None, (0, 6400), (6400, 12800)):
        ctx = _ctx(cs, 2)
        try:
            col = cs.Column(P, 9.8, Tl, 0.029, 0.0, 0.0, *_lorentz_synthetic(cs, ctx, nu), core=cs.Discretized(5, 2), nu_range=rng, ctx=ctx)
            col.run()
            Fup, Fdn = col.fetch()
            w = col.work()
            assert all(w[c] > 0 for c in MATRIX[:2]), (rng, _matrix_work(w))      # (up to 1e5 Pa a group's widest state leaves no 3-term part)
            F.append((np.array(Fup), np.array(Fdn)))
        finally:
            ctx.close()
    fm = np.abs(F[0][0]).max()
    for q in (0, 1):
        assert np.max(np.abs(F[1][q] + F[2][q] - F[0][q])) < 5e-13 * fm, q


# ---- e. state chunks -------------------------------------------------------------------------------------------------------------------------------

def test_state_chunks_bitwise(cs):
    """cs_shape_batch of code 1 on test_gpu_state_chunks' 400 000-line table: three chunks or more, the last with a partly filled group
    (boundaries()), the matrix cores forced.  The chunk driver runs each chunk as a call of its own states, so the rows are bitwise those
    of the same states called chunk by chunk (each such call fits one chunk)"""
    sl = cs.SpectralLines.synthetic(1, CH.NLINES, 11, 0.0, 25000.0)
    nu = CH.GRID_CO2
    n = CH.states_for("shape", CH.NLINES, len(nu))
    kc, b0 = CH.boundaries("shape", n, CH.NLINES, len(nu))
    Tk, P, Pp = CH._states(n, 101)
    ctx = _ctx(cs, 2)
    try:
        whole = cs.shape_batch(sl, "lorentz", nu, Tk, P, Pp, 25.0, ctx)
        parts = np.concatenate([cs.shape_batch(sl, "lorentz", nu, Tk[a:a + kc], P[a:a + kc], Pp[a:a + kc], 25.0, ctx) for a in [0] + b0])
    finally:
        ctx.close()
    assert whole.shape == (n, len(nu)) and np.all(whole > 0)
    assert np.array_equal(whole, parts)
    off = _ctx(cs, 0)
    try:
        rows = CH._check_rows(n, b0, 1)
        vec = cs.shape_batch(sl, "lorentz", nu, Tk[rows], P[rows], Pp[rows], 25.0, off)
    finally:
        off.close()
    _close_max(whole[rows], vec)
    print(f"{n} states in chunks of {kc}: bitwise the chunks' own calls; {len(rows)} rows against the vector unit")


# ---- f. what must not move -------------------------------------------------------------------------------------------------------------------------

def test_shifted_group_keeps_the_vector_path(cs):
    """code 1 | CS_SHAPE_PSHIFT (the CO2 fixture's own shifts): no matrix work, and bitwise the same under matrix-cores-2 and matrix-cores-0"""
    sl, nu = W.lines("fixture", "CO2"), SW.NU_A
    assert sl.delta_a is not None and np.any(sl.delta_a != 0.0)
    P = cs.pressuregrid(10.0, 1e5, 9)
    Tl = W.earth_temperature(P)
    got = {}
    for mc in (2, 0):
        ctx = _ctx(cs, mc)
        try:
            col = cs.Column(P, 9.8, Tl, 0.029, 0.0, 0.0, cs.DirectGas(sl, 1e-3, nu, shape="lorentz", pressure_shift=True), core=cs.Discretized(5, 2), ctx=ctx)
            r = SW.outputs(col)
            assert all(r["work"][c] == 0 for c in MATRIX) and r["work"]["dispatch"]["tables"] == 0, (mc, _matrix_work(r["work"]))
            got[mc] = r
        finally:
            ctx.close()
    assert np.max(got[2]["sigma"]) > 0
    for k in ("sigma", "tau", "Mup", "Mdn", "Fup", "Fdn"):
        assert np.array_equal(got[2][k], got[0][k]), k


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_resident_walk_bitwise(cs, O, graph):
    """a resident Lorentz column walked A -> B -> C -> A (test_gpu_state_walk's states), the matrix cores forced, eager and as a captured
    step (CS_TUNE_GRAPH): every step bitwise a fresh column's, the second visit to A bitwise the first, the oracle at 1e-11"""
    spec = SW.Spec(SW.NU_A, 9, SW.fixtures("lorentz", "lorentz"), tune=((4, int(graph)),), setup=SW.matrix_cores)
    Ts = SW.states(cs.pressuregrid(spec.Pt, 1e5, spec.npl))
    ctx = spec.context(cs)
    try:
        col = spec.column(cs, ctx, Ts["A"], SW.MU["A"])
        seen, worst = {}, {}
        for step, s in enumerate("ABCA"):
            if step:
                col.update(Ts[s], SW.MU[s])
            r = SW.outputs(col)
            assert r["work"]["node_evals_matrix"] > 0, (s, _matrix_work(r["work"]))
            _no_voigt_work(r["work"], r["info"], s)
            if s in seen:
                SW.same_as(r, seen[s], True, f"second visit to {s}")
                continue
            f = SW.fresh(cs, spec, Ts[s], SW.MU[s])
            SW.same_as(r, f, bool(np.array_equal(f["Fup"], SW.fresh(cs, spec, Ts[s], SW.MU[s])["Fup"])), f"step {step} ({s}) against a fresh column")
            SW.vs_oracle(cs, O, spec, col, r, worst)
            seen[s] = r
        assert seen["B"]["work"]["node_evals_matrix"] != seen["A"]["work"]["node_evals_matrix"]      # (other widths, other pieces)
    finally:
        ctx.close()
    print("walk", "graph" if graph else "eager", worst)
    assert all(v < 1e-11 for v in worst.values()), worst


def test_work_is_the_plan_that_ran(cs):
    """test_gpu_work_record's rule for a Lorentz column: work() after a run describes that run, also after the settings were changed
    behind it; the next run follows the new settings and, put back, counts what it counted"""
    cfg = W.config("C3", nnu=2001, nu_span=(600.0, 650.0), shape="lorentz")
    ctx = _ctx(cs, 2)
    try:
        col = cs.Column(cfg["P"], cfg["g"], cfg["T"], cfg["mu"], 0.0, 0.0, *cfg["absorbers"], core=cfg["core"], ctx=ctx)
        col.run()
        w0 = col.work()
        assert all(w0[c] > 0 for c in MATRIX) and w0["dispatch"]["tables"] != 0, w0
        strip = lambda w: {k: v for k, v in w.items() if k != "flux_scan_ns"}
        for apply, restore, moved in ((lambda: ctx.set_matrix_cores(0), lambda: ctx.set_matrix_cores(2), lambda w: w["node_evals_matrix"] == 0 and w["dispatch"]["tables"] == 0),
                                      (lambda: ctx.set_tuning(22, 1), lambda: ctx.set_tuning(22, 0), lambda w: w["dispatch"]["far_split"] == 1),
                                      (lambda: ctx.set_tuning(21, 1), lambda: ctx.set_tuning(21, 0), lambda w: w["dispatch"]["tables"] == 2)):
            apply()
            assert strip(col.work()) == strip(w0)
            col.run()
            assert moved(col.work()), col.work()
            restore()
            col.run()
            assert strip(col.work()) == strip(w0)
    finally:
        ctx.close()
