"""Column.work() describes the run as it was dispatched, not the settings in force when it is asked.

cs_column_work counts, on the host, what the last run issued -- from the zone tables that run left on the device and from the plan the
run was dispatched by (one VoigtPlan per Voigt group, kept in the column).  So a setting changed after the run must not show in the
counters until the column runs again, and a column that runs again under the new setting must count what a column set up under that
setting from the start counts.

The column is the one of tests/test_gpu_sub_lean.py -- C3 spacing, 2001 points over (600, 650), K = 61, 32 tiles with a ragged last
one, matrix cores forced on -- the smallest in which the matrix-core node sums, the window ends, the sub-tile cores and the range-only
pass are all in use.  Everything compared is an integer: no tolerance.  `flux_scan_ns` holds time stamps and is left out."""
import pytest

import workloads as W
from clearsky_jl_amd import DISPATCH_FLAGS

pytestmark = pytest.mark.gpu

# the settings cs_column_work once read live, each changed alone: (name, apply, restore)
_key = lambda k, v, d: (f"key{k}={v}", lambda ctx: ctx.set_tuning(k, v), lambda ctx: ctx.set_tuning(k, d))
SETTINGS = [_key(1, 1, 1), _key(6, 2, 0), _key(11, 1, 0), _key(14, 1, 0), _key(17, 1, 0), _key(18, 1, 0), _key(23, 1, 0),
            ("matrix_cores=0", lambda ctx: ctx.set_matrix_cores(0), lambda ctx: ctx.set_matrix_cores(2)),
            ("mixed", lambda ctx: ctx.set_precision("mixed"), lambda ctx: ctx.set_precision("fp64"))]
NAMES = [s[0] for s in SETTINGS]


def _work(col):
    w = col.work()
    del w["flux_scan_ns"]
    return w


def _column(cs, apply=None):
    ctx = cs.Context(0)
    ctx.set_matrix_cores(2)
    if apply:
        apply(ctx)
    cfg = W.config("C3", nnu=2001, nu_span=(600.0, 650.0))
    return ctx, cs.Column(cfg["P"], cfg["g"], cfg["T"], cfg["mu"], 0.0, 0.0, *cfg["absorbers"], core=cfg["core"], ctx=ctx)


_walked = {}


def _walk(cs):
    """One column: run, then for each setting -- change it, ask (stale), run and ask again (rerun), put it back, run and ask (back).
    Computed once for the tests that share it."""
    if not _walked:
        ctx, col = _column(cs)
        try:
            col.run()
            _walked["w0"] = _work(col)
            for name, apply, restore in SETTINGS:
                apply(ctx)
                stale = _work(col)
                col.run()
                rerun = _work(col)
                restore(ctx)
                col.run()
                _walked[name] = dict(stale=stale, rerun=rerun, back=_work(col))
        finally:
            ctx.close()
    return _walked


def test_column_uses_every_counted_kernel(cs):
    w0 = _walk(cs)["w0"]
    print({k: w0[k] for k in ("node_evals_matrix", "edge_mx_flops_issued", "sub_evals", "sub_lean_evals")}, w0["dispatch"])
    assert w0["node_evals_matrix"] > 0
    assert w0["edge_mx_flops_issued"] > 0
    assert w0["sub_evals"] > 0
    assert 0 < w0["sub_lean_evals"] < w0["sub_evals"]
    assert w0["dispatch"]["tables"] != 0


@pytest.mark.parametrize("name", NAMES)
def test_work_ignores_settings_changed_after_the_run(cs, name):
    r = _walk(cs)
    w0, stale, back = r["w0"], r[name]["stale"], r[name]["back"]
    assert stale == w0, {k: (w0[k], stale[k]) for k in w0 if stale[k] != w0[k]}
    assert back == w0, {k: (w0[k], back[k]) for k in w0 if back[k] != w0[k]}      # (and the same run again counts the same)


def test_the_settings_reach_the_dispatch(cs):
    """after the column has run again: the counters the setting governs have moved (so `stale == w0` above is not vacuous)"""
    r = _walk(cs)
    w0 = r["w0"]
    off = r["matrix_cores=0"]["rerun"]
    assert off["node_evals_matrix"] == 0 and off["sub_lean_evals"] == 0
    assert off["direct_evals_matrix"] == 0 and off["sub_evals"] == 0 and off["edge_mx_flops_issued"] == 0 and off["dispatch"]["tables"] == 0
    assert off["direct_evals"] > w0["direct_evals"] and off["node_evals"] == w0["node_evals"]    # (the vector unit took what the matrix cores had)
    full = r["key18=1"]["rerun"]                                     # the full loop in every wave of k_voigt_sub
    assert full["sub_lean_evals"] == 0 and full["sub_evals"] == w0["sub_evals"]
    # 32 tiles x 4 state groups: every item of k_cheb_nodes_mx is shared by the four waves of its block, so key 17 puts every far piece
    # on all 64 nodes and says so; key 11 does the same for want of the matrices -- never fewer flops issued than on 16 or 32 nodes
    shared = r["key17=1"]["rerun"]
    assert shared["dispatch"]["flags"] & DISPATCH_FLAGS["FAR64_SHARED"] and not w0["dispatch"]["flags"] & DISPATCH_FLAGS["FAR64_SHARED"]
    for name in ("key17=1", "key11=1"):
        assert r[name]["rerun"]["nodes_mx_flops_issued"] >= w0["nodes_mx_flops_issued"], name
        assert r[name]["rerun"]["node_evals_matrix"] == w0["node_evals_matrix"], name
    assert r["key17=1"]["rerun"]["nodes_mx_flops_issued"] == r["key11=1"]["rerun"]["nodes_mx_flops_issued"]


@pytest.mark.parametrize("name", NAMES)
def test_same_counters_as_a_column_set_up_under_the_setting(cs, name):
    rerun = _walk(cs)[name]["rerun"]
    ctx, col = _column(cs, SETTINGS[NAMES.index(name)][1])
    try:
        col.run()
        fresh = _work(col)
    finally:
        ctx.close()
    assert fresh == rerun, {k: (rerun[k], fresh[k]) for k in rerun if fresh[k] != rerun[k]}
