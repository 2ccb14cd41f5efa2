"""Every documented value of every lab switch (cs_set_tuning, cs_set_matrix_cores) dispatches and computes what it did when
tests/golden/tuning_record.json was recorded -- on the commit before the switches became one Settings record with one decoder.

Main column: the one of tests/test_gpu_work_record.py (C3 spacing, 2001 points over (600, 650), K = 61, matrix cores forced on).  Keys 9
and 10 act on PHCO2 only and run on the column "col/first" of tests/phco2_line_ref.py, the smallest there that Column.info() reports
k_phco2 for.  Each setting runs alone in a fresh Context and Column, three times (key 4 captures its graph on the second run and replays
it on the third); then Column.work() without `flux_scan_ns` (time stamps), Column.info() and the SHA-256 of sigma_nodes() and of the band
fluxes are held to the record: integers and hashes, no tolerance.  The record was taken twice and repeated in every field, hashes
included.  About half of the settings leave this column's record as the default's (key 1 = 0 with the matrix cores forced on, A/B forms that
compute the same bits, switches whose rule this grid size does not reach): tests/test_gpu_dispatch.py has both sides of each of their rules;
here they are held to change nothing.  Key 15 | 32 acts only in cs_fluxes_discretized_multi (tests/test_gpu_distributed.py).

PHCO2, every way in (recorded on the commit before a PHCO2 group's dispatch became one plan and its built levels got one key; taken twice,
both takes alike in every field).  The four columns of tests/phco2_line_ref.py under every run of P.RUNS, a snapshot after each of three
runs; col/graph also with key 4 on -- eager, captured, replayed, then updated to 296 K everywhere and back, three runs after each (the
update changes the regions the levels carry).  Every case of P.Cases under each of its runs through cs_shape_batch and cs_shape_points,
the whole array hashed; one cs_bake of a PHCO2 gas on the base grid, read back through cs_table_eval at two (T, P); cs_column_batch of
col/first with B = 3 (its own states, 296 K everywhere, col/graph's); and a sequence of cs_shape_batch calls in ONE context that changes
the cut-off, the grid and the region mask and comes back, each call held to the fresh-context hash of its case.  Every such call names a
new grid, so what holds the other fields of the levels' key are two columns, whose grid keeps its name: col/first run in one context
under one setting of keys 9 and 10 after another, each run held to the fresh-context record of that setting (the rules in the key), and a
column of two PHCO2 groups with cut-offs 500 and 200, which build the levels for each other on every step (the cut-off in the key).
record["provenance"] names the library the PHCO2 parts were taken on by its cs_build_id (the hash of its sources: _lib.source_id at that
commit); `PYTHONPATH=. python tests/test_gpu_tuning_record.py` takes them again, twice, and prints them."""
import hashlib
import json
import os

import numpy as np
import pytest

import phco2_line_ref as P
import workloads as W
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RECORD = os.path.join(GOLDEN, "tuning_record.json")

MAIN = {0: [1], 1: [0], 2: [0, 1], 3: [15, 100], 4: [1], 5: [0], 6: [2], 7: [0, 2], 8: [1, 16], 11: [1], 12: [1, 2], 13: [1, 2], 14: [1],
        15: [1, 2, 2 | 4, 2 | 8, 16, 128, 256, 2 | 1024, 2 | 2048], 16: [1, 2, 4], 17: [1], 18: [1, 2], 19: [1], 21: [1, 2], 22: [1, 2, 4],
        23: [1]}
MATRIX_CORES = [0, 1, 2 | 4]
PHCO2 = {9: [1], 10: [1, 2, 3]}

# (column, name, key or None for cs_set_matrix_cores, value); "default" changes nothing
SETTINGS = [("main", "default", None, None)] + [("main", f"key{k}={v}", k, v) for k, vs in MAIN.items() for v in vs]
SETTINGS += [("main", f"matrix_cores={v}", None, v) for v in MATRIX_CORES]
SETTINGS += [("phco2", "default", None, None)] + [("phco2", f"key{k}={v}", k, v) for k, vs in PHCO2.items() for v in vs]
IDS = [f"{c}-{n}" for c, n, _, _ in SETTINGS]


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


_inputs = {}


def _column(cs, which, ctx):
    if which == "main":
        if which not in _inputs:
            _inputs[which] = W.config("C3", nnu=2001, nu_span=(600.0, 650.0))
        cfg = _inputs[which]
        return cs.Column(cfg["P"], cfg["g"], cfg["T"], cfg["mu"], 0.0, 0.0, *cfg["absorbers"], core=cfg["core"], ctx=ctx)
    if which not in _inputs:
        nu = P.grids()["base"]
        Pl, Tl, _ = P.column_states(cs, P.COLUMN_K, P.COLUMN_SEED["col/first"])
        _inputs[which] = (nu, P.line_table(cs, [float(nu[50 * 64 + 32]) + 0.007]), Pl, Tl)
    nu, sl, Pl, Tl = _inputs[which]
    gas = cs.DirectGas(sl, P.CONC, nu, shape="PHCO2", dnu_cut=500.0)
    return cs.Column(Pl, 9.8, Tl, 0.029, 0.0, 0.0, gas, core=cs.Discretized(3, 2), ctx=ctx)


def measure(cs, which, key, value):
    """one setting alone in a fresh Context and Column: dict(work, info, sigma, fluxes) after three runs"""
    ctx = cs.Context(0)
    try:
        if which == "main":
            ctx.set_matrix_cores(2)
        if key is not None:
            ctx.set_tuning(key, value)
        elif value is not None:
            ctx.set_matrix_cores(value)
        col = _column(cs, which, ctx)
        for _ in range(3):
            col.run()
        work, info = col.work(), col.info()
        del work["flux_scan_ns"]
        Fup, Fdn = col.fetch()
        return dict(work=work, info=info, fluxes=_sha(Fup, Fdn), sigma=_sha(col.sigma_nodes()))
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def record():
    with open(RECORD) as f:
        return json.load(f)


def test_the_phco2_column_runs_k_phco2(record):
    assert all(r["info"]["line_kernel"] == 2 for r in record["phco2"].values())


@pytest.mark.parametrize("which,name,key,value", SETTINGS, ids=IDS)
def test_setting_dispatches_and_computes_as_recorded(cs, record, which, name, key, value):
    want, got = record[which][name], measure(cs, which, key, value)
    for part in ("work", "info"):
        assert got[part] == want[part], (part, {k: (want[part][k], got[part][k]) for k in want[part] if got[part][k] != want[part][k]})
    assert got["sigma"] == want["sigma"] and got["fluxes"] == want["fluxes"]


def test_a_key_by_name_is_the_key_by_number(cs, record):
    """Context.set_tuning takes a name of clearsky_jl_amd.TUNING for the integer"""
    assert cs.TUNING["FAR_SPLIT"] == 22
    assert measure(cs, "main", "FAR_SPLIT", 1) == record["main"]["key22=1"]


# ---- PHCO2: columns, entry points of gas_states, cs_column_batch, one context across many keys ---------------------------------------------

PH_COLUMNS = ["col/first", "col/second", "col/cut-100", "col/graph"]
PH_RUNS = [r.name for r in P.RUNS]
PH_CASES = list(P.placements(P.grids())) + PH_COLUMNS
BAKE_AT = [(250.0, 1e4), (290.0, 5e4)]
# (case, cut-off and grid as the case has them) in call order: the same twice, another cut-off, another grid, another region mask, back
SEQUENCE = ["mid-tile", "mid-tile", "cut-200-pair", "geo-mid", "col/graph", "mid-tile"]


@pytest.fixture(scope="module")
def cases(cs):
    return P.Cases(cs)


def _snapshot(col):
    work, info = col.work(), col.info()
    del work["flux_scan_ns"]
    Fup, Fdn = col.fetch()
    return dict(work=work, info=info, fluxes=_sha(Fup, Fdn), sigma=_sha(col.sigma_nodes()))


def _ph_column(cs, case, name, ctx):
    Pl, Tl, _ = P.column_states(cs, P.COLUMN_K, P.COLUMN_SEED[name])
    gases = [cs.DirectGas(sl, P.CONC, case.nu, shape="PHCO2", dnu_cut=case.cut) if sl is case.table else cs.DirectGas(sl, P.CONC, case.nu)
             for sl in case.tables]
    return cs.Column(Pl, 9.8, Tl, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, 2), ctx=ctx), Pl, Tl


def measure_ph_column(cs, case, name, run, graph=False):
    """a snapshot after each of three runs; graph: key 4 on, then updated to 296 K everywhere and back, three runs after each"""
    ctx = run.context(cs)
    try:
        if graph:
            ctx.set_tuning(4, 1)
        col, Pl, Tl = _ph_column(cs, case, name, ctx)
        out = []
        for T in (None, np.full(len(Pl), 296.0), Tl) if graph else (None,):
            if T is not None:
                col.update(T)
            for _ in range(3):
                col.run()
                out.append(_snapshot(col))
        return out
    finally:
        ctx.close()


def measure_ph_entry(cs, case, run, ctx=None):
    """the SHA-256 of what cs_shape_batch and cs_shape_points return for the case's PHCO2 table at its states"""
    T, Pk = (np.array(x) for x in zip(*case.states))
    own = ctx is None
    ctx = run.context(cs) if own else ctx
    try:
        return dict(batch=_sha(cs.shape_batch(case.table, "PHCO2", case.nu, T, Pk, P.CONC * Pk, case.cut, ctx)),
                    points=_sha(cs.shape_points(case.table, "PHCO2", case.nu, T, Pk, P.CONC * Pk, case.cut, ctx)))
    finally:
        if own:
            ctx.close()


def measure_ph_bake(cs, case, run):
    ctx = run.context(cs)
    try:
        gas = cs.Gas(case.table, P.CONC, case.nu, cs.AtmosphericDomain((200.0, 300.0), 3, (1e3, 1e5), 3), shape="PHCO2", dnu_cut=case.cut, ctx=ctx)
        return _sha(*[gas.rawsigma(T, Pa) for T, Pa in BAKE_AT])
    finally:
        ctx.close()


def measure_ph_batch(cs, case, run):
    ctx = run.context(cs)
    try:
        col, Pl, Tl = _ph_column(cs, case, "col/first", ctx)
        return _sha(*col.run_batch([Tl, np.full(len(Pl), 296.0), P.column_states(cs, P.COLUMN_K, P.COLUMN_SEED["col/graph"])[1]]))
    finally:
        ctx.close()


def measure_ph_two_cuts(cs, case):
    """col/first's gas twice in one column, cut-offs 500 and 200: two PHCO2 groups on one grid; a snapshot after each of three runs"""
    ctx = P.RUN["default"].context(cs)
    try:
        Pl, Tl, _ = P.column_states(cs, P.COLUMN_K, P.COLUMN_SEED["col/first"])
        gases = [cs.DirectGas(case.table, P.CONC, case.nu, shape="PHCO2", dnu_cut=cut) for cut in (500.0, 200.0)]
        col = cs.Column(Pl, 9.8, Tl, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, 2), ctx=ctx)
        out = []
        for _ in range(3):
            col.run()
            out.append(_snapshot(col))
        return out
    finally:
        ctx.close()


def _same(got, want):
    for g, w in zip(got, want):
        for part in ("work", "info"):
            assert g[part] == w[part], (part, {k: (w[part][k], g[part][k]) for k in w[part] if g[part][k] != w[part][k]})
        assert g["sigma"] == w["sigma"] and g["fluxes"] == w["fluxes"]
    assert len(got) == len(want)


@pytest.mark.parametrize("run", PH_RUNS)
@pytest.mark.parametrize("name", PH_COLUMNS)
def test_phco2_column_as_recorded(cs, cases, record, name, run):
    _same(measure_ph_column(cs, cases[name], name, P.RUN[run]), record["ph_columns"][name][run])


@pytest.mark.parametrize("run", PH_RUNS)
def test_phco2_captured_column_as_recorded(cs, cases, record, run):
    """col/graph with key 4 on, across two changes of the region mask"""
    want = record["ph_graph"][run]
    assert len(want) == 9
    _same(measure_ph_column(cs, cases["col/graph"], "col/graph", P.RUN[run], graph=True), want)


@pytest.mark.parametrize("name", PH_CASES)
def test_phco2_shape_calls_as_recorded(cs, cases, record, name):
    runs = cases.runs(name)
    assert sorted(record["ph_entry"][name]) == sorted(r.name for r in runs)
    for run in runs:
        assert measure_ph_entry(cs, cases[name], run) == record["ph_entry"][name][run.name], run.name


def test_phco2_bake_and_column_batch_as_recorded(cs, cases, record):
    for run in P.RUNS:
        assert measure_ph_bake(cs, cases["mid-tile"], run) == record["ph_bake"][run.name], run.name
        assert measure_ph_batch(cs, cases["col/first"], run) == record["ph_batch"][run.name], run.name


def test_phco2_one_context_across_cut_offs_grids_and_masks(cs, cases, record):
    """what the levels were built for is one key: a call after another cut-off, grid or region mask computes what a fresh context does"""
    run = P.RUN["default"]
    ctx = run.context(cs)
    try:
        for n, name in enumerate(SEQUENCE):
            assert measure_ph_entry(cs, cases[name], run, ctx) == record["ph_entry"][name]["default"], (n, name)
    finally:
        ctx.close()


# settings of keys 9 and 10 in turn on ONE context and column, by the run of P.RUNS that has them
RULES_SEQUENCE = ["default", "nodes-64", "tiles-as-intervals", "own-core", "tiles-as-intervals-64", "default"]


def test_phco2_one_column_across_rules(cs, cases, record):
    """the grid keeps its name, so only the rules in the key tell the levels of one setting from the next: each run computes what a fresh
    context under that setting does"""
    ctx = P.RUN["default"].context(cs)
    try:
        col, _, _ = _ph_column(cs, cases["col/first"], "col/first", ctx)
        for n, name in enumerate(RULES_SEQUENCE):
            for key in (9, 10):
                ctx.set_tuning(key, P.RUN[name].tune.get(key, 0))
            col.run()
            want = record["ph_columns"]["col/first"][name][-1]
            Fup, Fdn = col.fetch()
            assert _sha(col.sigma_nodes()) == want["sigma"] and _sha(Fup, Fdn) == want["fluxes"], (n, name)
            assert col.info()["line_kernel"] == 2
    finally:
        ctx.close()


def test_phco2_two_cut_offs_in_one_column_as_recorded(cs, cases, record):
    _same(measure_ph_two_cuts(cs, cases["col/first"]), record["ph_two_cuts"]["default"])


def record_phco2(cs):
    """the PHCO2 parts of the record, as the tests above read them"""
    cases = P.Cases(cs)
    return dict(ph_columns={n: {r: measure_ph_column(cs, cases[n], n, P.RUN[r]) for r in PH_RUNS} for n in PH_COLUMNS},
                ph_graph={r: measure_ph_column(cs, cases["col/graph"], "col/graph", P.RUN[r], graph=True) for r in PH_RUNS},
                ph_entry={n: {r.name: measure_ph_entry(cs, cases[n], r) for r in cases.runs(n)} for n in PH_CASES},
                ph_bake={r.name: measure_ph_bake(cs, cases["mid-tile"], r) for r in P.RUNS},
                ph_batch={r.name: measure_ph_batch(cs, cases["col/first"], r) for r in P.RUNS},
                ph_two_cuts=dict(default=measure_ph_two_cuts(cs, cases["col/first"])),
                provenance=dict(phco2=dict(build_id=cs.lib().cs_build_id().decode(), takes=2)))


if __name__ == "__main__":
    import clearsky_jl_amd
    takes = [json.dumps(record_phco2(clearsky_jl_amd), sort_keys=True) for _ in range(2)]
    assert takes[0] == takes[1], "the two takes differ"
    print(takes[0])
