"""The matrix-core series radii at their 1e-15 bound (sep_radii, cs_kernels.h) on C3-spacing windows that hold the high-pressure states.

The 61 node states of the C3 column span 1 Pa .. 1e5 Pa; the windows are cut out of the bench grid at its own spacing (0.025 cm^-1) and
small enough for the oracle.  The default path and the matrix-core path forced on must agree with the all-vector path to 2e-14 (measured:
1.07e-14 and 9.1e-15; the 1e-17 radii gave 1.05e-14 and 9.0e-15 -- the vector bodies' own errors and the sum order, not the series) and
with the oracle to 1e-11, and must take the (line, node | point, state) work the shorter radii hand it: the counts are
those of the build at 1e-15 -- the 1e-17 radii left node sums 41.2 M / 39.1 M, 3-term evaluations 37.2 M / 29.8 M and sub-tile core pairs
1.91 M / 2.09 M on the two windows."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

# span: (node sums on the matrix cores at least, 3-term matrix evaluations at least, sub-tile core pairs at most) -- midway between
# the counts at the 1e-17 radii and at 1e-15 (43.9 M / 51.7 M / 1.60 M resp. 42.2 M / 45.9 M / 1.73 M)
SPANS = {(600.0, 650.0): (42.5e6, 44.4e6, 1.76e6), (1500.0, 1550.0): (40.6e6, 37.9e6, 1.90e6)}


def _run(cs, cfg, mc):
    ctx = cs.Context(0)
    try:
        if mc is not None:
            ctx.set_matrix_cores(mc)
        col = cs.Column(cfg["P"], cfg["g"], cfg["T"], cfg["mu"], 0.0, 0.0, *cfg["absorbers"], core=cfg["core"], ctx=ctx)
        col.run()
        return col, col.sigma_nodes(), col.work()
    finally:
        ctx.close()


@pytest.mark.parametrize("span", list(SPANS), ids=lambda s: f"{s[0]:g}-{s[1]:g}")
def test_radii_vs_vector_path_and_oracle(cs, O, span):
    import workloads as W
    cfg = W.config("C3", nnu=2001, nu_span=span)
    col, s_def, _ = _run(cs, cfg, None)
    _, s_mx, w_mx = _run(cs, cfg, 2)
    _, s_vec, w_vec = _run(cs, cfg, 0)
    assert col.K == 61 and w_vec["node_evals_matrix"] == 0 and w_vec["direct_evals_matrix"] == 0
    assert relerr(s_def, s_vec, floor=1e-280) <= 2e-14
    assert relerr(s_mx, s_vec, floor=1e-280) <= 2e-14
    ref = O.fluxes_discretized(cfg["nu"], cfg["P"], cfg["g"], 2, col.Tn, col.mun, col.Tlev, [g.sl for g in col.gases], ["voigt"] * 2,
                               [25.0] * 2, col.conc, want_sigma=True)
    for s in (s_def, s_mx):
        assert relerr(s, ref["sigma"], floor=1e-280) < 1e-11
    nodes_min, mx3_min, sub_max = SPANS[span]
    assert w_mx["node_evals_matrix"] >= nodes_min, w_mx["node_evals_matrix"]
    assert w_mx["matrix_evals_3term"] >= mx3_min, w_mx["matrix_evals_3term"]
    assert 0 < w_mx["sub_evals"] <= sub_max, w_mx["sub_evals"]
    assert w_mx["direct_evals"] < w_vec["direct_evals"] and w_mx["node_evals"] == w_vec["node_evals"]
