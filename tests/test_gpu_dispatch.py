"""The kernel forms one cs_column_run can dispatch, on both sides of every grid-size rule in cs_api.hip that selects them.

Each rule of RULES picks a form from a quantity of the grid (tiles, tiles x K, intervals x K, piece-table items).  For every rule the
grid just below and the grid at its threshold are built from the rule's formula -- K = nl (nlob - 1) + 1 states, 64-point tiles,
interval sizes from cs.interp_plan -- so that a moved threshold or formula fails here instead of silently leaving a form untested.  On
each side the test asserts the form the library reports (Column.work()["dispatch"], Column.info()), compares the column with the
oracle, and compares it with the other side's form forced by its cs_set_tuning key on the same grid: bitwise where the dev header says
"same results" / "same tables", else at 5e-13 (test_gpu_merge._close).  Then the switches no other test runs, and the edges that change
the padding of the matrix-core and sub-tile forms (K mod 16, ragged last tiles, a batch whose B x K crosses the far-split rule).

Oracle tolerances are the suite's: sigma and tau 1e-11 relative, M+- 1e-11 of their maximum, band fluxes 1e-11 of max F+.  Grids of up to
~20 000 points are compared whole, longer ones on a sample of wavenumbers (first and last tile whole, 64 random points in between).

The seeded synthetic tables of the bench workload (40 lines per cm^-1 together) keep every matrix-core piece in use.  The grid spacing,
0.008 cm^-1, lets the 4096-tile rule stay inside the tables' 1 .. 2500 cm^-1.
"""
import functools
import numpy as np
import pytest

import clearsky_jl_amd
import workloads as W
from conftest import relerr
from test_gpu_merge import _close

pytestmark = pytest.mark.gpu

NU0, DNU, CUT = 300.0, 0.008, 25.0
NP_DEF = 61                                       # levels: nl = 60, nlob = 2 -> K = 61


def _K(np_, nlob=2):
    return (np_ - 1) * (nlob - 1) + 1


def _nu(n):
    return NU0 + DNU * np.arange(n)


def _n_itot(n):
    """intervals over all levels of the plan (ChebGrid::nItot) for an n-point grid"""
    return sum(-(-n // s) for s in clearsky_jl_amd.interp_plan(_nu(n), CUT))


def _tiles(n):
    return -(-n // 64)


def _first_n(pred, lo, hi):
    """the smallest n in (lo, hi] with pred(n), pred monotone, pred(lo) false"""
    assert not pred(lo) and pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


def _disp(r):
    return r["work"]["dispatch"]


@functools.lru_cache(maxsize=3)
def _run(n, np_=NP_DEF, tune=(), first_level=-1, p_surf=1e5):
    """one column (synthetic H2O + CO2, Discretized(5, 2)) on an n-point grid with the given cs_set_tuning keys; every output"""
    cs = clearsky_jl_amd
    nu = _nu(n)
    P = cs.pressuregrid(10.0, p_surf, np_)
    T = W.earth_temperature(P)
    gases = (cs.DirectGas(W.lines("synthetic", "H2O"), W.fC_h2o, nu), cs.DirectGas(W.lines("synthetic", "CO2"), 400e-6, nu))
    ctx = cs.Context(0)
    try:
        if first_level != -1:
            ctx.set_interp_plan(first_level=first_level)
        for k, v in tune:
            ctx.set_tuning(k, v)
        col = cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=ctx)
        assert col.K == _K(np_)
        col.run()
        tau = np.zeros((col.nl, col.nnu), order="F")
        Mu = np.zeros((col.np, col.nnu), order="F")
        Md = np.zeros((col.np, col.nnu), order="F")
        Fup, Fdn = col.fetch(tau, Mu, Md)
        r = dict(sigma=col.sigma_nodes(), tau=tau, Mup=Mu, Mdn=Md, Fup=Fup, Fdn=Fdn, nu=col.nu, Tlev=col.Tlev, work=col.work(),
                 info=col.info(), col=col)
    finally:
        ctx.close()
    return r


def _vs_oracle(O, r):
    col, n = r["col"], len(r["nu"])
    if n <= 20000:
        idx = np.arange(n)
    else:
        last = n - ((n - 1) % 64 + 1)
        mid = np.random.default_rng(n).choice(np.arange(64, last), 64, replace=False)
        idx = np.unique(np.concatenate([np.arange(64), mid, np.arange(last, n)]))
    ref = O.fluxes_discretized(col.nu[idx], col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [g.sl for g in col.gases], ["voigt"] * 2,
                               [CUT] * 2, col.conc, want_sigma=True)
    assert relerr(r["sigma"][:, idx], ref["sigma"], floor=1e-280) < 1e-11
    assert relerr(r["tau"][:, idx], ref["tau"]) < 1e-11
    sm = max(ref["Mup"].max(), ref["Mdn"].max())
    for k in ("Mup", "Mdn"):
        assert np.max(np.abs(r[k][:, idx] - ref[k])) < 1e-11 * sm, k
    if n == len(idx):
        fm = ref["Fup"].max()
        for k in ("Fup", "Fdn"):
            assert np.max(np.abs(r[k] - ref[k])) < 1e-11 * fm, k


def _same(a, b, bitwise):
    if bitwise:
        for k in ("sigma", "tau", "Mup", "Mdn", "Fup", "Fdn"):
            assert np.array_equal(a[k], b[k]), k
    else:
        _close(a, b, 5e-13, 1e-12)


def _flag(bit):
    return lambda r: bool(_disp(r)["flags"] & bit)


def _nflag(bit):
    return lambda r: not _disp(r)["flags"] & bit


def _field(name, v):
    return lambda r: _disp(r)[name] == v


def _flux(v):
    return lambda r: r["info"]["flux_form"] == v


def _streams_near(on):
    return lambda r: bool(_disp(r)["streams"] & 2) == on


# Column.work()["dispatch"]["flags"] bits (CS_DF_* of include/clearsky_hip_dev.h)
TNODES, NEAR_MEMSET, RT_STREAMS, BAND_SUM, FAR64_SHARED, CHUNK4, CASCADE_ASIDE = (
    clearsky_jl_amd.DISPATCH_FLAGS[n] for n in ("TNODES", "NEAR_MEMSET", "RT_STREAMS", "BAND_SUM", "FAR64_SHARED", "CHUNK4", "CASCADE_ASIDE"))


def _by_tiles(thr, below_if_less=True):
    """grids of whole tiles: (largest tile count on the `below` side, the first on the other); `below_if_less`: the rule is
    `tiles < thr`, else `tiles <= thr`"""
    t = thr - 1 if below_if_less else thr
    return lambda K: (t, t + 1)


def _by_tile_states(thr, below_if_less=True):
    """the same for a rule on tiles x K"""
    def f(K):
        t = (thr - 1) // K if below_if_less else thr // K
        return t, t + 1
    return f


# One row per rule: (name, quantity, threshold, tile counts below / at (from K), form below, form at, key forcing the `at` form on the
# `below` grid, key forcing the `below` form on the `at` grid, bitwise, tuning both sides run with).  None: no key forces that form
# (the form is reached by its rule only).  Rules on intervals or piece-table items have their own tests below.
RULES = [
    ("far split 4 -> 2 waves per tile", "tiles*K", 4096, _by_tile_states(4096), _field("far_split", 4), _field("far_split", 2),
     ((22, 2),), ((22, 4),), False, ()),
    ("far split 2 -> 1 wave per tile", "tiles*K", 16384, _by_tile_states(16384), _field("far_split", 2), _field("far_split", 1),
     ((22, 1),), ((22, 2),), False, ()),
    ("near-line side stream from 8192 tile-states", "tiles*K", 8192, _by_tile_states(8192), _streams_near(False), _streams_near(True),
     ((7, 2),), ((7, 0),), False, ()),
    ("k_rt_streams up to 400 tiles (flux kernels unfused: key 15 = 1)", "tiles", 400, _by_tiles(400, False), _flag(RT_STREAMS),
     _nflag(RT_STREAMS), ((5, 0),), None, False, ((15, 1),)),
    ("in-kernel band sum up to 512 flux blocks (scan form: a block per tile)", "tiles", 512, _by_tiles(512, False), _flag(BAND_SUM),
     _nflag(BAND_SUM), ((15, 4),), None, False, ()),
    ("window ends on 16 tile nodes from 1024 (tile, state group) blocks", "tiles*ceil(K/16)", 1024, lambda K: _by_tiles(1024 // -(-K // 16))(K),
     _nflag(TNODES), _flag(TNODES), None, ((23, 1),), False, ()),
    ("near-line priority from 512 tiles", "tiles", 512, _by_tiles(512), _field("near_prio", 0), _field("near_prio", 3),
     ((16, 2),), ((16, 1),), True, ()),
    ("piece tables merged below 1024 tiles", "tiles", 1024, _by_tiles(1024), _field("tables", 1), _field("tables", 2),
     ((21, 1),), ((21, 2),), True, ()),
    ("scan flux form up to 1024 tiles", "tiles", 1024, _by_tiles(1024, False), _flux(3), _flux(0),
     ((15, 1),), ((15, 1024),), False, ()),
    ("chunk flux form from 4096 tiles (rt_geometry: one wave per tile)", "tiles", 4096, _by_tiles(4096), _flux(0), _flux(2),
     ((15, 2),), ((15, 1),), False, ()),
]
# Not in the table: sep_in_use / edge_in_use (mx_big at 2048 (interval, group) and 1024 (tile, group) blocks) decide nothing by
# default -- cs_set_tuning key 1 = 1 keeps the matrix-core kernels on short grids -- and key 1 = 0 is compared in test_gpu_merge;
# flux_plan's 65536-point rule only changes k_rt's tiles per block (not reported; the grids of the scan rule sit on it).


def _grids(rule):
    """(n below, n at): a full last tile below, a last tile of one point at the threshold"""
    tb, ta = rule[3](_K(NP_DEF))
    return 64 * tb, 64 * (ta - 1) + 1


@pytest.mark.parametrize("rule", RULES, ids=[r[0] for r in RULES])
def test_threshold_matrix(O, rule):
    name, qty, thr, _, below, at, force_at, force_below, bitwise, base = rule
    K = _K(NP_DEF)
    nb, na = _grids(rule)
    q = {"tiles": _tiles, "tiles*K": lambda n: _tiles(n) * K, "tiles*ceil(K/16)": lambda n: _tiles(n) * -(-K // 16)}[qty]
    assert q(nb) < thr <= q(na) or q(nb) <= thr < q(na), (name, q(nb), q(na))
    base = tuple(base)
    rb, ra = _run(nb, tune=base), _run(na, tune=base)
    assert below(rb), (name, "below", _disp(rb), rb["info"])
    assert at(ra), (name, "at", _disp(ra), ra["info"])
    for r, force, want in ((rb, force_at, at), (ra, force_below, below)):
        _vs_oracle(O, r)
        if force is None:
            continue
        f = _run(len(r["nu"]), tune=base + tuple(force))
        assert want(f), (name, "forced", force, _disp(f), f["info"])
        _same(f, r, bitwise)


def test_near_stream_upper_bound_by_states(O):
    """the near-line side stream up to 300 000 (tile, state) waves: 1000 tiles at K = 300 (on) and K = 301 (off); the other side's form
    forced by key 7 on each"""
    t = 1000
    for np_, on in ((300000 // t, True), (300000 // t + 1, False)):
        assert (t * _K(np_) <= 300000) == on
        r = _run(64 * t, np_)
        assert bool(_disp(r)["streams"] & 2) == on, _disp(r)
        _vs_oracle(O, r)
        f = _run(64 * t, np_, ((7, 0 if on else 2),))
        assert bool(_disp(f)["streams"] & 2) != on
        _same(f, r, False)


def test_node_kernel_split_below_16384_waves(O):
    """k_cheb_nodes with four waves per (interval, state) below 16384 (interval, state) waves, one wave per four states at and above;
    every level in use (first_level 0), so the intervals are all of the plan's; key 13 forces the other form on each grid"""
    K = _K(NP_DEF)
    na = _first_n(lambda n: _n_itot(n) * K >= 16384, 1000, 400000)
    for n, split in ((na - 1, 1), (na, 0)):
        r = _run(n, first_level=0)
        assert r["work"]["intervals"] == _n_itot(n)
        assert _disp(r)["nodes_split"] == split, (n, _disp(r))
        _vs_oracle(O, r)
        f = _run(n, tune=((13, 2 if split else 1),), first_level=0)
        assert _disp(f)["nodes_split"] == 1 - split
        _same(f, r, False)


def test_piece_tables_one_thread_above_50000_items(O):
    """one thread per piece-table item above 50 000 items (intervals + tiles, times state groups): the smallest column that reaches
    them on this grid spacing at K = 256; below it the sixteen-lane kernel (k_mxzones16), whose tables key 15 | 16 makes by one thread
    per item bitwise alike"""
    np_ = 256
    g = -(-_K(np_) // 16)
    items = lambda n: g * (_n_itot(n) + _tiles(n))
    na = _first_n(lambda n: items(n) > 50000, 70000, 400000)
    rb, ra = _run(na - 1, np_, first_level=0), _run(na, np_, first_level=0)
    assert _tiles(na - 1) >= 1024
    assert _disp(rb)["tables"] == 2 and _disp(ra)["tables"] == 3, (_disp(rb), _disp(ra))
    for r in (rb, ra):
        _vs_oracle(O, r)
    f = _run(na - 1, np_, ((15, 16),), first_level=0)
    assert _disp(f)["tables"] == 3
    _same(f, rb, True)


# the three builds of the matrix-core piece tables, each forced by its key: (tuning, Column.work()["dispatch"]["tables"])
TABLE_FORMS = ((((21, 2),), 1), (((21, 1),), 2), (((15, 16),), 3))


def _work_but_form(r):
    """Column.work() without the two fields that may differ between the forms: which form ran, and the flux kernel's time stamps"""
    w = dict(r["work"])
    del w["flux_scan_ns"]
    w["dispatch"] = {k: v for k, v in w["dispatch"].items() if k != "tables"}
    return w


@pytest.mark.parametrize("np_,p_surf,tiles,min_states", [(17, 5e3, 40, (None,)), (40, 1e5, 420, (None, 1, 16))], ids=["K17", "K40"])
def test_piece_table_forms_same_tables(np_, p_surf, tiles, min_states):
    """the piece tables as blocks of k_gas_setup_mx (key 21 = 2), by k_mxzones16 (key 21 = 1) and by k_mxzones (key 15 = 16) on one short
    grid of whole tiles and a last tile of ONE point (the core test's "all 64 points present" clause decides there), with the matrix-core
    kernels kept on it (key 1 = 1): bitwise equal outputs, and equal work counts -- cs_column_work counts from the tables it reads back, so
    every piece bound of both tables enters them.  K = 17: a second state group of ONE state (its rank clamped to it); K = 40: a
    half-filled second group (one octet of the lean bits has no state), also with key 8 (min_states) at 1 and at 16.  The counts that
    must not be zero keep the comparison from being one between empty tables.

    Grids.  K = 40: n = 64 * 419 + 1.  On 40 tiles (300 .. 320 cm^-1) no tile has a lean bit at any key 8 (sub_lean_evals 0 with
    core_tile_states 624, matrix_evals_3term 17 465 344); lengthened in whole tiles the first bits come at 418 tiles (sub_lean_evals 0 at
    417, 3584 at 418, 10 240 at 420: the Doppler widths grow with the wavenumber), so 420.
    K = 17: n = 64 * 39 + 1, on levels from 10 Pa to 5e3 Pa instead of the file's 1e5 Pa.  A tile's core and the 3-term split go by the
    group's WIDEST state (edge_pieces): a core needs its 8-term radius, 8.66 x its largest Lorentz width, below 0.3 x the tile's
    0.504 cm^-1, so a width below 0.0175 cm^-1 -- pressures below some 1.5e4 Pa for the tables' widths of up to 0.1 cm^-1 / atm.  With 17
    levels up to 1e5 Pa the first group's sixteenth state lies at 9.2e4 Pa and the second group is the surface state, so no tile of any
    grid length has a core there (core_tile_states = matrix_evals_3term = 0 on 40, 80, 160, 320, 640, 1000, 1500, 2000, 3000 and 4000
    tiles, the last reaching the end of the line tables; node_evals_matrix 8 724 736, direct_evals_matrix 2 517 632 on 40).  Up to
    5e3 Pa the widest width is 0.1 x 5e3 / 101325 x (296 / 200)^0.8 < 0.007 cm^-1: both groups, the one of ONE state too, have a
    core on each of the 39 whole tiles (core_tile_states 663 = 39 x 17, matrix_evals_3term 9 992 448, node_evals_matrix 10 022 464,
    direct_evals_matrix 4 781 760)"""
    n = 64 * (tiles - 1) + 1
    first, lean = [], []
    for ms in min_states:
        base = ((1, 1),) + (((8, ms),) if ms is not None else ())
        runs = [_run(n, np_, base + tune, p_surf=p_surf) for tune, _ in TABLE_FORMS]
        for r, (tune, form) in zip(runs, TABLE_FORMS):
            assert _disp(r)["tables"] == form, (tune, _disp(r))
        for r in runs[1:]:
            _same(r, runs[0], True)
            assert _work_but_form(r) == _work_but_form(runs[0]), (ms, _disp(r))
        w = runs[0]["work"]
        print(f"K = {np_}, {tiles} tiles, min_states {ms}: node_evals_matrix {w['node_evals_matrix']}, direct_evals_matrix {w['direct_evals_matrix']}, "
              f"core_tile_states {w['core_tile_states']}, matrix_evals_3term {w['matrix_evals_3term']}, sub_lean_evals {w['sub_lean_evals']}")
        first.append(w)
        lean.append(w["sub_lean_evals"])
    for w in first:
        assert w["node_evals_matrix"] > 0 and w["direct_evals_matrix"] > 0, w
        assert w["core_tile_states"] > 0 and w["matrix_evals_3term"] > 0, w
    if np_ == 40:
        assert max(lean) > 0, lean


# The switches no other test compares with the defaults, each on a grid where it changes what runs: (tuning, grid in tiles, what the
# default runs, what the switch runs, bitwise).  Keys 21 and 22 (every value) and 15 | 1024 are in the threshold matrix above.
SWITCHES = [
    ({17: 1}, 135, _nflag(FAR64_SHARED), _flag(FAR64_SHARED), False),
    ({19: 1}, 135, _nflag(NEAR_MEMSET), _flag(NEAR_MEMSET), True),
    ({15: 8}, 4096, lambda r: _flux(2)(r) and _nflag(CHUNK4)(r), _flag(CHUNK4), False),
    ({15: 256}, 400, _flag(CASCADE_ASIDE), _nflag(CASCADE_ASIDE), False),
    ({15: 128}, 512, lambda r: _flux(3)(r) and r["work"]["flux_scan_ns"][4] == 0, lambda r: r["work"]["flux_scan_ns"][4] > 0, True),
]


@pytest.mark.parametrize("sw", SWITCHES, ids=[str(s[0]) for s in SWITCHES])
def test_untested_switches_same_results(sw):
    tune, t, dflt, forced, bitwise = sw
    n = 64 * t
    a, b = _run(n), _run(n, tune=tuple(tune.items()))
    assert dflt(a), (tune, _disp(a), a["info"])
    assert forced(b), (tune, _disp(b), b["info"])
    _same(b, a, bitwise)


@pytest.mark.parametrize("np_,last", [(64, 63), (65, 1), (63, 63), (66, 1)])
def test_padding_edges_vs_oracle(O, np_, last):
    """K = 64, 65, 63 (0, 1, 15 mod 16) and 65 states (a group of one): padded state groups of the matrix-core pieces and of
    k_voigt_sub's sub-tiles; last tiles of 63 and 1 points; on grids where the tile nodes, the merged piece tables and the near-line
    stream are in use"""
    n = 64 * 299 + last
    r = _run(n, np_)
    d = _disp(r)
    assert d["tables"] == 1 and d["streams"] & 2 and d["flags"] & TNODES, d
    _vs_oracle(O, r)


def test_batch_crosses_far_split(cs, O):
    """one cs_column_batch of B = 2 columns of 67 tiles at K = 61: B x K x tiles crosses the 4096-wave far-split rule (2 waves per tile)
    that the single column (4 per tile) does not -- against the same columns run one by one and against the oracle"""
    K = _K(NP_DEF)
    t = (4096 - 1) // K
    assert t * K < 4096 <= 2 * t * K
    n = 64 * t
    nu = _nu(n)
    P = cs.pressuregrid(10.0, 1e5, NP_DEF)
    T0 = W.earth_temperature(P)
    Ts = [T0, T0 + np.linspace(-4.0, 6.0, len(P))]
    gases = (cs.DirectGas(W.lines("synthetic", "H2O"), W.fC_h2o, nu), cs.DirectGas(W.lines("synthetic", "CO2"), 400e-6, nu))
    ctx = cs.Context(0)
    col = cs.Column(P, 9.8, T0, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(5, 2), ctx=ctx)
    Fu, Fd = col.run_batch(Ts, 0.029)
    assert col.work()["dispatch"]["far_split"] == 2
    for b, T in enumerate(Ts):
        col.update(T, 0.029)
        col.run()
        a = col.fetch()
        assert col.work()["dispatch"]["far_split"] == 4
        fm = a[0].max()
        assert np.max(np.abs(Fu[b] - a[0])) < 1e-13 * fm and np.max(np.abs(Fd[b] - a[1])) < 1e-13 * fm
        ref = O.fluxes_discretized(nu, P, 9.8, 2, col.Tn, col.mun, col.Tlev, [g.sl for g in col.gases], ["voigt"] * 2, [CUT] * 2,
                                   col.conc)
        fm = ref["Fup"].max()
        assert np.max(np.abs(Fu[b] - ref["Fup"])) < 1e-11 * fm and np.max(np.abs(Fd[b] - ref["Fdn"])) < 1e-11 * fm
    ctx.close()
