"""Every evaluation form of the PHCO2 line sum (shape code 3) on ISOLATED lines against 40-digit values (tests/phco2_line_ref.py, which
derives the probes, classifies each by the form that serves it and builds both bounds; tests/test_phco2_line_ref.py checks on the host what
is presupposed here, the oracle under the same bounds included).

A probe is within the cut-off of one line only, so what the device returns there is one line's term as one form evaluated it: the six
region-uniform sets of k_phco2 with the 2- and the 4-term body, its four boundary sets on either side of their boundary, the cut-off edge
segments, the core through the inner Voigt pass (3 cm^-1 cut-off) with k_phco2's halves beside it or through its own loop (cs_set_tuning
key 9), every virtual level of k_phco2_nodes (16, 32, 64 nodes; key 10 = 1, 2, 3) with the own range below and above the parent's, and
k_linesum off the fast path (cut-off 100, tiles wider than 27 cm^-1) -- through cs_shape_batch, cs_shape_points and a 17-level column with
the PHCO2 gas first or second, interpolation on and off, at 25, 100, 143, 144, 296 and 1000 K (chi > 1 below 143.6 K), 1 .. 3e6 Pa.
Every probe is held to the hard bound (lineparam_bound(C0_GPU) with the chi term, about 2.1e-13) and, at s >= 1e3, to the sharp bound
(3e-14 .. 6e-14); the 40-digit zeros beyond the cut-off must be exact zeros; interpolation on and off must agree within the sum of their
bounds.  No probe is left out of a comparison (the host test asserts that none is of the underflow class).  The plan and the region mask
the classification rests on are held to the library's own under every setting (test_plan_and_mask_are_the_library_s), a column's
launch count shows the node kernels ran, and a captured step (key 4) is replayed across a change of the mask.

Recorded figures (MI355X; 415 comparisons of 56 cases; worst error / bound over the probes a form group serves, hard | sharp;
printed when the module ends; node groups are (node count, region, own range below / above the parent's), sizes and sides merged):
  uniform sets   region 1  2-term 0.054 | 0.372   4-term 0.047 | 0.333      boundary sets  120 left   near 0.033 | 0.146   far 0.034 | 0.232
                 region 2  2-term 0.066 | 0.388   4-term 0.057 | 0.357                      30 left   near 0.044 | 0.246   far 0.037 | 0.308
                 region 3  2-term 0.063 | 0.326   4-term 0.042 | 0.261                      30 right  near 0.047 | 0.277   far 0.037 | 0.288
  cut-off edges  left 0.022 | 0.107   right 0.025 | 0.150                                  120 right  near 0.021 | 0.156   far 0.034 | 0.216
  core           inner Voigt pass 0.060 | 0.410   halves 0.038 | 0.257   own loop: near 0.058 | 0.356, far 0.038 | 0.228
  k_linesum      0.028 | 0.480
  nodes  16: region 2 low 0.034 | 0.249  high 0.038 | 0.220   region 3 low 0.062 | 0.342  high 0.038 | 0.229
         32: region 1 low 0.050 | 0.277  high 0.057 | 0.417   region 2 low 0.050 | 0.370  high 0.041 | 0.311   region 3 low 0.044 | 0.307  high 0.043 | 0.207
         64: region 1 low 0.050 | 0.359  high 0.044 | 0.259   region 2 low 0.045 | 0.315  high 0.042 | 0.257   region 3 low 0.066 | 0.328  high 0.046 | 0.245
All <= 1.  The states below 143.6 K (chi > 1) are among them: the 2-term body, whose zone bound takes the unscaled y, stays at 0.39 of the
sharp bound -- it keeps every term through u^2 and needs s >= 1e6 only (phco2_line_ref).

One finding, fixed in the library.  "margin-32" first held a 25 K, 3e6 Pa state (now the case margin-32-cold): its line, just beyond 30 cm^-1
below a 2048-point interval, came out 4.9e-12 wrong at 49 probes of that state (22 x the hard bound) with interpolation on and inside the
bounds with it off.  gamma = 12 cm^-1 and chi up to 4.5 put a zero of the profile's denominator x^2 + (chi y)^2 -- d = +-i gamma chi(d) --
35 cm^-1 from the centre and 20 above the real axis, over that interval, and 32 nodes cannot resolve it; ph_levels' node counts take the line
centre for the nearest singularity.  ph_wide_regions (cs_api.hip) now keeps a region out of the levels of a launch whose states let those
zeros reach a tenth of the region's near distance towards the real axis; such calls sum the region per point (0.373 of the sharp bound).
The dense-table tests at 2e-11 and 5e-13 never held a state below 160 K.  The rule is cautious (its range: test_wide_states_keep_regions_out
of the host module; region 2 goes at 143 .. 165 K at 3e6 Pa too).  At its limit: a 25 K state at 0.95 of the region-2 limit, interpolated on
32 nodes from the same position, 0.060 | 0.323 (margin-32-edge); at 0.95 of the region-1 limit on 64 nodes 0.048 | 0.301 (margin-64-edge);
at 1.05 of the region-2 limit, per point, 0.062 | 0.332 (margin-32-over).  A captured step (key 4) replayed across the update of a warm
column to col/graph's states: 0.048 | 0.298 in the eager, the captured and the replayed run after it.

Seeded defects (a scratch build per change, never committed), each caught -- the first failing test and its worst error / bound:
  boundary sets, gn / gf swapped                mid-tile, hard: 9e11 (0.21 relative at 31 cm^-1)
  boundary sets, rn[b] for both sides           mid-tile, hard: 9e11
  fabs(dv) >= 3.0 in the inner-Voigt halves     mid-tile, hard: 5e12 (the probes at exactly 3.0 cm^-1 counted twice: error 1.0)
  parent clamp dropped in k_phco2_nodes         mid-tile, hard: 2e13 (600 probes, up to 4 x the value)
  pos <= cnt in ph_segment_lds                  mid-tile, hard: 1e13 (640 probes)
  fR[0] = fL[0]                                 mid-tile, hard: 3e11 (214 probes on the right of the line)
  two[r] always true                            high-mid, sharp: 2.16 (4.4e-14 at s = 6.8e4; at 640 cm^-1 region 1 starts at s >= 1e6, where
                                                both bodies are inside 1e-15 -- only a grid at 6400 cm^-1, ten times the Doppler width, has
                                                region-1 lines below s = 1e6 for two[r] to matter)
"""
import numpy as np
import pytest

import phco2_line_ref as P

pytestmark = pytest.mark.gpu

_WORST = {}        # form group -> [worst / hard, worst / sharp]


def _group(fm):
    if fm[0] == "node":
        return ("node", fm[2], fm[3], fm[5])             # node count, region, piece (sizes and sides merged)
    if fm[0] == "uniform":
        return ("uniform", fm[1], fm[3])
    return fm


def _note(per):
    for fm, (h, s) in per.items():
        w = _WORST.setdefault(_group(fm), [0.0, 0.0])
        w[0], w[1] = max(w[0], h), max(w[1], s)


@pytest.fixture(scope="module")
def cases(cs):
    yield P.Cases(cs)
    # the figures of the module docstring: worst error / bound per form group over the comparisons this module ran (compare() has held
    # every one of them to 1)
    for g in sorted(_WORST, key=str):
        print(f"  {str(g):44s} {_WORST[g][0]:.3f} | {_WORST[g][1]:.3f}")


def test_plan_and_mask_are_the_library_s(cs, cases):
    """what phco2_line_ref classifies probes by is what the library plans: under every run's settings (interpolation off, cs_set_tuning key
    10 = 1, 2, 3) and with every set of regions kept out, Context.phco2_plan gives the restated levels on every grid and cut-off; the
    regions a case's states keep out are cs.phco2_wide_regions of them"""
    drops = [(), (1,), (2,), (1, 2), (1, 2, 3)]
    for run in P.RUNS:
        ctx = run.context(cs)
        try:
            for gname, nu in cases.grids.items():
                for cut in P.CUTS:
                    for drop in drops:
                        want = [(s, nc, regs) for s, nc, regs, _ in P.levels(nu, cut, run.interp, run.force64, drop=frozenset(drop))[1]]
                        assert ctx.phco2_plan(nu, cut, drop) == want, (run.name, gname, cut, drop)
            assert (ctx.phco2_plan(cases.grids["base"], 500.0) == []) == (not run.interp)
        finally:
            ctx.close()
    for name in cases.names():
        c = cases[name]
        T, g = [c.states[k][0] for k in range(c.K)], [c.gbound(k) for k in range(c.K)]
        assert set(cs.phco2_wide_regions(T, g, c.cut)) == set(P.wide_regions(list(zip(T, g)), c.cut)), name


def _names():
    import clearsky_jl_amd
    return list(P.Cases(clearsky_jl_amd).place)


def _batch(cs, case, run):
    T, Pk = (np.array(x) for x in zip(*case.states))
    ctx = run.context(cs)
    try:
        a = cs.shape_batch(case.table, "PHCO2", case.nu, T, Pk, P.CONC * Pk, case.cut, ctx)
        b = cs.shape_points(case.table, "PHCO2", case.nu, T, Pk, P.CONC * Pk, case.cut, ctx)
    finally:
        ctx.close()
    return a, b


@pytest.mark.parametrize("name", _names())
def test_batch_and_points(cs, cases, name):
    """one call of K = 1, 5 or 17 states through cs_shape_batch and cs_shape_points under every run of the case: both bounds at every probe,
    exact zeros beyond the cut-off; interpolation on against off within the sum of their bounds"""
    case = cases[name].reference()
    assert len(case.pr) <= P.MAX_PROBES and case.K in P.K_SETS
    failed, kept = [], {}
    for run in cases.runs(name):
        a, b = _batch(cs, case, run)
        for what, got, strict in (("batch", a, True), ("points", b, False)):
            if strict and case.points_only:
                # the line at exactly the cut-off from an end point: the strict end-point pre-filter of the vector method drops it
                if not (np.all(got == 0.0) and np.sum(~case.zero) == len(case.ksel) and np.all(b[case.k, case.i][~case.zero] > 0.0)):
                    failed.append(f"{run.name} {what}: the strict pre-filter")
                continue
            try:
                wh, ws, per = P.compare(case, got[case.k, case.i], run, f"{name} {run.name} {what}", strict=strict)
                _note(per)
                print(f"{name} {run.name} {what}: {len(case.pr)} probes, worst error / bound  hard {wh:.3f}  sharp {ws:.3f}")
            except AssertionError as e:
                failed.append(f"{run.name} {what}: {e}")
            kept[(run.name, what)] = got[case.k, case.i]
    if ("default", "batch") in kept and ("interp-off", "batch") in kept:
        for what, strict in (("batch", True), ("points", False)):
            on, off = kept[("default", what)], kept[("interp-off", what)]
            b_on, m_on, s_on, _ = case.bounds(P.RUN["default"], strict=strict)
            b_off, m_off, s_off, _ = case.bounds(P.RUN["interp-off"], strict=strict)
            lim = (np.where(m_on, s_on, b_on) + np.where(m_off, s_off, b_off)) * np.abs(case.want)
            if not (np.all(np.abs(on - off) <= lim) and np.array_equal(on == 0.0, off == 0.0)):
                q = int(np.argmax(np.abs(on - off) / np.where(lim > 0, lim, 1.0)))
                failed.append(f"interpolation on vs off, {what}: probe {case.pr[q]} differs by {abs(on[q] - off[q]) / case.want[q]:.3e}, allowed {lim[q] / case.want[q]:.3e}")
    assert not failed, "\n".join(failed)


COLUMNS = [("col/first", 2), ("col/second", 2), ("col/cut-100", 1), ("col/graph", 2)]


@pytest.mark.parametrize("name,kernel", COLUMNS, ids=[c[0] for c in COLUMNS])
def test_column(cs, cases, name, kernel):
    """a 17-level column (1 Pa .. 3e6 Pa, the six temperatures in turn) whose PHCO2 gas comes first (base + extra) or second behind a
    Voigt gas (accumulate), and one at cut-off 100 (k_linesum): Column.info()["line_kernel"] names the kernel, five states at every probe"""
    case = cases[name].reference()
    Pl, Tl, sts = P.column_states(cs, P.COLUMN_K, P.COLUMN_SEED[name])
    failed, launches = [], {}
    for run in cases.runs(name):
        ctx = run.context(cs)
        try:
            gases = [cs.DirectGas(sl, P.CONC, case.nu, shape="PHCO2", dnu_cut=case.cut) if sl is case.table else cs.DirectGas(sl, P.CONC, case.nu)
                     for sl in case.tables]
            col = cs.Column(Pl, 9.8, Tl, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, 2), ctx=ctx)
            assert col.K == case.K and np.array_equal(col.Tk, [s[0] for s in sts]) and np.array_equal(col.Pk, [s[1] for s in sts])
            col.run()
            got, info = col.sigma_nodes()[case.k, case.i], col.info()
        finally:
            ctx.close()
        launches[run.name] = info["launches"]
        if info["line_kernel"] != kernel:
            failed.append(f"{run.name}: line_kernel {info['line_kernel']}")
        try:
            wh, ws, per = P.compare(case, got, run, f"{name} {run.name}", strict=False)
            _note(per)
            print(f"{name} {run.name}: {len(case.pr)} probes, worst error / bound  hard {wh:.3f}  sharp {ws:.3f}")
        except AssertionError as e:
            failed.append(f"{run.name}: {e}")
    # the levels really ran: the node sums and their carry to the grid are launches of their own (none off the fast path)
    assert (launches["default"] > launches["interp-off"]) == (kernel == 2), launches
    assert not failed, "\n".join(failed)


def test_graph_replay_across_a_change_of_regions(cs, cases):
    """cs_set_tuning key 4: a step captured while every state is warm (296 K: every region on the levels) and replayed, then the column
    updated to col/graph's states, whose last is 25 K at 3e6 Pa (regions 1 and 2 off the levels: the line sits where 32 nodes left 4.9e-12) --
    the update drops the captured step, and the next runs (eager, captured, replayed) are held to the same bounds as an eager column.
    cs_column_sigma_fetch evaluates the cross-sections again where the step finished them on chip, so what the replayed launches
    themselves wrote is read from the optical depths: they must be, bit for bit, those of a column set up eagerly in the cold states (the same
    launches on the same inputs).  Without the invalidation (a scratch build) the first replay after the update differs by 2.2e-14 -- the
    warm plan's 4.9e-12 in the 25 K state, diluted by the 1000 K state of the same layer -- and the next by 1.8e7: it reads levels that the
    evaluation in between has laid out anew"""
    case = cases["col/graph"].reference()
    Pl, Tl, sts = P.column_states(cs, P.COLUMN_K, P.COLUMN_SEED["col/graph"])
    run = P.RUN["default"]

    def tau_of(col):
        tau = np.zeros((col.nl, col.nnu), order="F")
        col.fetch(tau)
        return tau

    ctx = run.context(cs)
    try:
        gas = cs.DirectGas(case.table, P.CONC, case.nu, shape="PHCO2", dnu_cut=case.cut)
        col = cs.Column(Pl, 9.8, Tl, 0.029, 0.0, 0.0, gas, core=cs.Discretized(3, 2), ctx=ctx)
        col.run()
        eager = tau_of(col)
    finally:
        ctx.close()
    assert np.all(np.isfinite(eager)) and np.all(eager > 0.0)
    ctx = run.context(cs)
    ctx.set_tuning(4, 1)
    try:
        gas = cs.DirectGas(case.table, P.CONC, case.nu, shape="PHCO2", dnu_cut=case.cut)
        col = cs.Column(Pl, 9.8, np.full(len(Pl), 296.0), 0.029, 0.0, 0.0, gas, core=cs.Discretized(3, 2), ctx=ctx)
        warm = []
        for _ in range(3):           # eager, captured, replayed
            col.run()
            warm.append(col.sigma_nodes()[case.k, case.i])
        assert np.array_equal(warm[0], warm[1]) and np.array_equal(warm[0], warm[2])
        col.update(Tl)
        assert np.array_equal(col.Tk, [s[0] for s in sts]) and np.array_equal(col.Pk, [s[1] for s in sts])
        cold = []
        for n in range(3):
            col.run()
            diff = float(np.max(np.abs(tau_of(col) - eager) / eager))
            print(f"col/graph run {n} after the update: optical depths against the eager column {diff:.2e}")
            assert diff == 0.0, (n, diff)
            cold.append(col.sigma_nodes()[case.k, case.i])
            wh, ws, _ = P.compare(case, cold[-1], run, f"col/graph after the update, run {n}", strict=False)
            print(f"col/graph run {n} after the update: worst error / bound  hard {wh:.3f}  sharp {ws:.3f}")
        assert np.array_equal(cold[0], cold[1]) and np.array_equal(cold[0], cold[2])
        col.update(np.full(len(Pl), 296.0))      # and back: the levels carry every region again, same values as before
        col.run()
        assert np.array_equal(col.sigma_nodes()[case.k, case.i], warm[0])
    finally:
        ctx.close()
