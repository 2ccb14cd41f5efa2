"""The range-only pass of k_voigt_sub (cs_set_tuning key 18, include/clearsky_hip_dev.h) on C3-spacing windows with the 61 node states.

A wave of k_voigt_sub whose octet of states the piece tables mark as unable to reach the six-term series inside the core radius
(EdgeZone::lean) sums nothing: it forms the hand-off ranges only and, had it met a series pair after all, would run the full loop.
Every skipped addition is `acc += 0.0`, so key 0 (by the tables), 1 (full loop everywhere, the behaviour before the pass existed) and
2 (range-only first in every wave: the fall-back everywhere a series pair exists) must give the same bits in the cross-sections, the
optical depths, M+, M-, F+ and F-.

Windows (as test_gpu_series_radii.py: 2001 points at the bench grid's spacing, matrix cores forced on so that short grids have cores):
(600, 650) and (1500, 1550) -- the two low-pressure state groups predicted free of series pairs, the third not; (1, 51) -- Doppler
widths are tiny there, y^2 large, and nu - cut <= 0 on the lower tiles: waves of the low groups are predicted to reach the series or
find out on the way.  Against the yardsticks of test_gpu_series_radii.py: 2e-14 to the all-vector path, 1e-11 to the oracle."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

KEY = 18
SPANS = [(600.0, 650.0), (1500.0, 1550.0), (1.0, 51.0)]
_ids = lambda s: f"{s[0]:g}-{s[1]:g}"


def _column(cs, cfg, absorbers, mc, lean):
    """one step; (col, sigma at the nodes, tau, M+, M-, F+, F-, work)"""
    ctx = cs.Context(0)
    try:
        ctx.set_matrix_cores(mc)
        ctx.set_tuning(KEY, lean)
        col = cs.Column(cfg["P"], cfg["g"], cfg["T"], cfg["mu"], 0.0, 0.0, *absorbers, core=cfg["core"], ctx=ctx)
        col.run()
        tau = np.zeros((col.nl, col.nnu), order="F")
        Mup, Mdn = np.zeros((col.np, col.nnu), order="F"), np.zeros((col.np, col.nnu), order="F")
        Fup, Fdn = col.fetch(tau, Mup, Mdn)
        return col, dict(sigma=col.sigma_nodes(), tau=tau, Mup=Mup, Mdn=Mdn, Fup=Fup, Fdn=Fdn), col.work()
    finally:
        ctx.close()


_runs = {}


def _three(cs, span):
    """the window at key 0, 1 and 2, computed once for the tests that share it"""
    if span not in _runs:
        import workloads as W
        cfg = W.config("C3", nnu=2001, nu_span=span)
        _runs[span] = (cfg, [_column(cs, cfg, cfg["absorbers"], 2, lean) for lean in (0, 1, 2)])
    return _runs[span]


def _same_bits(runs, what):
    for lean in (1, 2):
        for name, a in runs[0][1].items():
            assert np.array_equal(a, runs[lean][1][name]), f"{what}: {name} differs between key {KEY} = 0 and {lean}"


@pytest.mark.parametrize("span", SPANS, ids=_ids)
def test_same_bits_at_every_setting(cs, span):
    cfg, runs = _three(cs, span)
    assert runs[0][0].K == 61
    for lean, (_, out, w) in enumerate(runs):
        print(f"{span} key {KEY} = {lean}: sub_evals {w['sub_evals']} sub_lean_evals {w['sub_lean_evals']} max sigma {out['sigma'].max():.6e}")
        assert np.all(np.isfinite(out["sigma"])) and out["sigma"].max() > 0.0
    _same_bits(runs, span)


@pytest.mark.parametrize("span", SPANS[:2], ids=_ids)
def test_range_only_pass_ran(cs, span):
    _, runs = _three(cs, span)
    w0, w1 = runs[0][2], runs[1][2]
    print(f"{span}: sub_lean_evals / sub_evals = {w0['sub_lean_evals']} / {w0['sub_evals']} = {w0['sub_lean_evals'] / max(w0['sub_evals'], 1):.4f}")
    assert 0 < w0["sub_lean_evals"] < w0["sub_evals"], (w0["sub_lean_evals"], w0["sub_evals"])
    assert w1["sub_lean_evals"] == 0 and w1["sub_evals"] == w0["sub_evals"], (w1["sub_lean_evals"], w1["sub_evals"], w0["sub_evals"])


@pytest.mark.parametrize("span", SPANS[:2], ids=_ids)
def test_vs_vector_path_and_oracle(cs, O, span):
    cfg, runs = _three(cs, span)
    col, out, _ = runs[0]
    _, vec, w_vec = _column(cs, cfg, cfg["absorbers"], 0, 0)
    assert w_vec["direct_evals_matrix"] == 0 and w_vec["sub_evals"] == 0
    e_vec = relerr(out["sigma"], vec["sigma"], floor=1e-280)
    ref = O.fluxes_discretized(cfg["nu"], cfg["P"], cfg["g"], 2, col.Tn, col.mun, col.Tlev, [g.sl for g in col.gases], ["voigt"] * 2,
                               [25.0] * 2, col.conc, want_sigma=True)
    e_ref = relerr(out["sigma"], ref["sigma"], floor=1e-280)
    print(f"{span}: sigma vs all-vector path {e_vec:.3e}, vs oracle {e_ref:.3e}")
    assert e_vec <= 2e-14
    assert e_ref < 1e-11


def test_same_bits_beside_a_vvh_group(cs):
    """H2O as shape code 5 (voigtVVH: its records carry S~, the kernel is the same) beside CO2 as plain Voigt"""
    import workloads as W
    span = (600.0, 650.0)
    cfg = W.config("C3", nnu=2001, nu_span=span)
    h2o, co2 = cfg["absorbers"]
    mixed = [cs.DirectGas(h2o.sl, W.fC_h2o, cfg["nu"], shape="voigtVVH"), co2]
    runs = [_column(cs, cfg, mixed, 2, lean) for lean in (0, 1, 2)]
    for lean, (_, out, w) in enumerate(runs):
        print(f"VVH + Voigt, key {KEY} = {lean}: sub_evals {w['sub_evals']} sub_lean_evals {w['sub_lean_evals']}")
        assert np.all(np.isfinite(out["sigma"])) and out["sigma"].max() > 0.0
    _same_bits(runs, "VVH + Voigt")
