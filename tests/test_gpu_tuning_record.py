"""Every documented value of every lab switch (cs_set_tuning, cs_set_matrix_cores) dispatches and computes what it did when
tests/golden/tuning_record.json was recorded -- on the commit before the switches became one Settings record with one decoder.

Main column: the one of tests/test_gpu_work_record.py (C3 spacing, 2001 points over (600, 650), K = 61, matrix cores forced on).  Keys 9
and 10 act on PHCO2 only and run on the column "col/first" of tests/phco2_line_ref.py, the smallest there that Column.info() reports
k_phco2 for.  Each setting runs alone in a fresh Context and Column, three times (key 4 captures its graph on the second run and replays
it on the third); then Column.work() without `flux_scan_ns` (time stamps), Column.info() and the SHA-256 of sigma_nodes() and of the band
fluxes are held to the record: integers and hashes, no tolerance.  The record was taken twice and repeated in every field, hashes
included.  About half of the settings leave this column's record as the default's (key 1 = 0 with the matrix cores forced on, A/B forms that
compute the same bits, switches whose rule this grid size does not reach): tests/test_gpu_dispatch.py has both sides of each of their rules;
here they are held to change nothing.  Key 15 | 32 acts only in cs_fluxes_discretized_multi (tests/test_gpu_distributed.py)."""
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
