"""Host tests of tests/phco2_line_ref.py: what tests/test_gpu_phco2_line.py presupposes of its inputs, its probes, its classification and
its two bounds, checked without a GPU -- chi is continuous, the restated ph_levels is the library's on every grid, the grids provide the
levels asked of them, every probe sees one line, no test holds more than MAX_PROBES and none is of the underflow class, the placements
sit where the rules put them, every evaluation form is reached by a probe with a non-zero 40-digit value, and the oracle
(oracle/cs_oracle.c: the scalar form of the model) meets both bounds at the device's probes before the device is held to them."""
import math

import mpmath as mp
import numpy as np
import pytest

import lineparam_ref as R
import phco2_line_ref as P


@pytest.fixture(scope="module")
def cases(cs):
    return P.Cases(cs)


def test_chi_continuous_and_above_one_when_cold():
    """at |dnu| = 3, 30, 120 the 40-digit chi of the formula below and of the formula above agree to 1e-38 at every temperature of T_SET;
    B1 changes sign between 143 and 144 K, and below it chi > 1 throughout region 1 and into region 2 (about 4.5 at 30 cm^-1 at 25 K)"""
    for T in P.T_SET:
        for D in R.PH_D:
            lo, hi = R.chi_phco2(mp.mpf(D), T, -1), R.chi_phco2(mp.mpf(D), T, +1)
            assert lo[1] + 1 == hi[1] and abs(lo[0] - hi[0]) <= mp.mpf(10) ** -38 * hi[0], (T, D)
        assert R.chi_phco2(mp.mpf("2.999"), T)[:2] == (mp.mpf(1), 0)
    assert R.ph_coefs(143.0)[0] < 0 < R.ph_coefs(144.0)[0]
    assert 4.4 < R.chi_phco2(mp.mpf(30), 25.0)[0] < 4.6 and R.chi_phco2(mp.mpf(55), 25.0)[0] > 1 > R.chi_phco2(mp.mpf(65), 25.0)[0]
    assert all(R.chi_phco2(mp.mpf(d), 143.0)[0] > 1 for d in (3.5, 29.0, 30.0)) and all(R.chi_phco2(mp.mpf(d), 144.0)[0] < 1 for d in (3.5, 29.0))


def test_plans(cs, cases):
    """the restated ph_levels is cs.phco2_plan on every grid and cut-off used, and the grids provide what the cases rely on: levels of 16, 32
    and 64 nodes; every region at two or more sizes, each but the largest with the next larger size as its parent (par[] never jumps a
    size: phco2_line_ref); interval widths that differ along the geometric grid and move its node counts; no levels below 128 points,
    with interpolation off, or off the fast path"""
    g = cases.grids
    for name, nu in g.items():
        for cut in P.CUTS:
            sizes, vl, fine = P.levels(nu, cut)
            assert [(s, nc, regs) for s, nc, regs, _ in vl] == cs.phco2_plan(nu, cut), (name, cut)
    sizes, vl, fine = P.levels(g["base"], 500.0)
    assert len(g["base"]) == 6417 and I_tiles(g["base"]) == 101 and len(g["base"]) % 64 == 17
    assert {nc for _, nc, _, _ in vl} == {16, 32, 64} and sizes == [8192, 4096, 2048, 1024, 512, 256, 128]
    for r in (1, 2, 3):
        carried = [s for s, _, regs, _ in vl if r in regs]
        assert len(carried) >= 2 and fine[r] == 128, (r, carried)
        assert len({nc for _, nc, regs, _ in vl if r in regs}) >= 2          # (more than one node count per region along the sizes)
    for name in ("base", "low", "geo"):
        for cut in (500.0, 200.0):
            sizes, vl, _ = P.levels(g[name], cut)
            for s, _, regs, par in vl:
                for r in regs:
                    above = [x for x, _, rg, _ in vl if x > s and r in rg]
                    assert par[r] == (min(above) if above else None), (name, cut, s, r)
                    assert not above or par[r] == 2 * s, (name, cut, s, r)      # never a jump
    w = np.diff(g["geo"])
    assert w[-1] / w[0] > 1.3 and [(s, nc, regs) for s, nc, regs, _ in P.levels(g["geo"], 500.0)[1]] != [(s, nc, regs) for s, nc, regs, _ in vl]
    assert cs.phco2_plan(g["short"], 500.0) == [] and len(g["short"]) < 128
    assert P.levels(g["base"], 500.0, interp=False)[1] == []
    # the runs: key 10 bit 0 gives 64 nodes everywhere, bit 1 the tiles as 64-point intervals
    assert {nc for _, nc, _, _ in P.levels(g["base"], 500.0, force64=1)[1]} == {64}
    assert P.levels(g["base"], 500.0, force64=2)[0][-1] == 64 and {nc for _, nc, _, _ in P.levels(g["base"], 500.0, force64=3)[1]} == {64}
    mu = cases["mid-tile"].table.mu
    assert P.fast_ok(g["base"], 500.0, mu.min()) and P.fast_ok(g["base"], 200.0, mu.min()) and P.fast_ok(g["low"], 500.0, mu.min())
    assert not P.fast_ok(g["base"], 100.0, mu.min()) and not P.fast_ok(g["wide"], 500.0, mu.min())
    assert max(g["wide"][min(i + 63, len(g["wide"]) - 1)] - g["wide"][i] for i in range(0, len(g["wide"]), 64)) > 27.0
    assert g["low"][-1] - 500.0 <= 0.0                                      # (no tile of the low grid has a lower bound on the Doppler width)


def test_wide_states_keep_regions_out(cs, cases):
    """ph_wide_regions: the restated rule is the library's (cs.phco2_wide_regions) over a sweep of temperatures and widths; which states it
    touches with the tables' widths (gamma_air 0.07, n 0.7) -- at 3e6 Pa regions 1 and 2 at 25 and 100 K, region 2 alone at 143 and 144 K
    (up to 165 K), nothing at 296 and 1000 K; at 1e5 Pa only 25 K; nothing below 1e4 Pa -- and with gamma_air = 0.1 region 1 at 296 K,
    3e6 Pa; the calm cases keep nothing out, the edge cases sit at 0.95 and 1.05 of a limit; on the high grid region 1 takes the 4-term
    body at 1000 K (two[r] false)"""
    for T in (25.0, 60.0, 100.0, 130.0, 143.0, 144.0, 160.0, 170.0, 200.0, 296.0, 600.0, 1000.0):
        for g in 10.0 ** np.linspace(-6, 1.5, 46):
            for cut in (500.0, 200.0):
                assert set(cs.phco2_wide_regions([T], [g], cut)) == set(P.wide_regions([(T, float(g))], cut)), (T, g, cut)
    assert set(cs.phco2_wide_regions([296.0, 25.0], [0.01, 0.5])) == {1, 2}          # (one wide state of a call is enough)
    at = lambda T, Pk: set(P.wide_regions([(T, P.gamma_of(T, Pk))], 500.0))
    corner = {25.0: {1, 2}, 100.0: {1, 2}, 143.0: {2}, 144.0: {2}, 296.0: set(), 1000.0: set()}
    for T, want in corner.items():
        assert at(T, P.P_HI) == want, (T, at(T, P.P_HI))
        assert at(T, 1e5) == ({1, 2} if T == 25.0 else set()) and at(T, 1e4) == set(), T
    assert at(165.0, P.P_HI) == {2} and at(170.0, P.P_HI) == set() and at(100.0, 1e6) == {2}
    wider = (P.KTREF / 296.0) ** 0.7 * 0.1 * P.P_HI / P.KATM                   # gamma_air = 0.1 at 296 K, 3e6 Pa
    assert set(P.wide_regions([(296.0, wider)], 500.0)) == {1} and set(P.wide_regions([(1000.0, wider * (296.0 / 1000.0) ** 0.7)], 500.0)) == set()
    ref = cases["mid-tile"]
    assert abs(P.gamma_of(*ref.states[16]) * (1.0 + 1e-12) / ref.gbound(16) - 1.0) < 1e-12
    drop = lambda c: set(P.wide_regions([(c.states[k][0], c.gbound(k)) for k in range(c.K)], c.cut))
    for name in ("mid-tile", "geo-mid", "col/first", "margin-16", "margin-32", "margin-64"):
        c = cases[name]
        assert drop(c) == set() and {r for _, _, regs, _ in c.geometry(P.RUN["default"]).vl for r in regs} == {1, 2, 3}, name
    assert any(T >= 296.0 and Pk > 2e6 for T, Pk in ref.states) and any(T == 25.0 for T, _ in ref.states)
    for name, want, r, x in (("margin-32-edge", {1}, 2, 0.95), ("margin-64-edge", set(), 1, 0.95), ("margin-32-over", {1, 2}, 2, 1.05)):
        c = cases[name]
        k = c.K - 2
        assert k in c.ksel and c.states[k][0] == 25.0 and abs(P.wide_reach(25.0, c.gbound(k), 500.0)[r - 1] / x - 1.0) < 1e-6, name
        assert drop(c) == want, (name, drop(c))
    for name, size, nc, r, i0 in (("margin-32-edge", 2048, 32, 2, 2048), ("margin-64-edge", 512, 64, 1, 2048)):
        assert cases[name].geometry(P.RUN["default"]).node_form(i0 // 64, 0)[1:4] == (size, nc, r), name
    c = cases["margin-32-cold"]
    assert c.states[4][0] == 25.0 and abs(c.states[4][1] - P.P_HI) < 1e-6 and 4 in c.ksel
    g = c.geometry(P.RUN["default"])
    assert drop(c) == {1, 2} and {r for _, _, regs, _ in g.vl for r in regs} == {3}
    assert all(fm[0] != "node" or fm[3] == 3 for fm in c.reference().forms(P.RUN["default"]))
    for name in ("col/second", "col/graph", "geo-mid-cold", "margin-32-over"):
        assert drop(cases[name]) == {1, 2}, name
    assert cases["col/graph"].states[16] == (25.0, cases["col/graph"].states[16][1]) and abs(cases["col/graph"].states[16][1] - P.P_HI) < 1e-6
    h = cases["high-mid"]
    assert h.states[0][0] == 1000.0 and 0 in h.ksel and h.geometry(P.RUN["default"]).fast
    gh = h.geometry(P.RUN["default"])
    assert not gh.node_two(128, 50 * 64 // 128 + 1, 1, 1000.0, h.gbound(0)) and gh.zone_q(50, 1000.0, h.gbound(0))[2] > 3.0


def I_tiles(nu):
    return -(-len(nu) // 64)


def test_placements_sit_on_the_rules(cases):
    """exact distances are exact, the cut-off edges cross tiles, the margins are just beyond max(D_r, margin h), the clusters put the real
    line at every index asked, the state sets are 1, 5 and 17 with every temperature compared, cold and thick states included"""
    b = cases.grids["base"]
    pl = cases.place
    for D in (3.0, 30.0, 120.0):
        for side, sg in (("left", 1.0), ("right", -1.0)):
            c = pl[f"exact-{D:g}-{side}"][1][0]
            hit = np.nonzero((b - c) * sg == D)[0]
            assert hit.size == 1, (D, side)
            case = cases[f"exact-{D:g}-{side}"]
            assert (0, int(hit[0]), 0) in case.pr
    assert b[0] - pl["exactly-cut-lo"][1][0] == 500.0 and pl["exactly-cut-hi-200"][1][0] - b[-1] == 200.0
    for name, sg in (("edge-lo", 1.0), ("edge-hi", -1.0)):
        e = pl[name][1][0] + sg * 500.0
        i = int(np.searchsorted(b, e))
        assert 0 < i < len(b) and (i - 1) // 64 == i // 64 and i % 64 not in (0, 63), name      # inside a tile
    c1, c2 = pl["cut-200-pair"][1]
    assert c2 - c1 > 2 * 200.0 and b[0] < c1 + 200.0 < b[-1] and b[0] < c2 - 200.0 < b[-1]
    sizes, vl, _ = P.levels(b, 500.0)
    nc_of = {(s, r): nc for s, nc, regs, _ in vl for r in regs}
    assert nc_of[(1024, 3)] == 16 and nc_of[(2048, 2)] == 32 and nc_of[(512, 1)] == 64
    for name, size, r, i0 in (("margin-16", 1024, 3, 3072), ("margin-32", 2048, 2, 2048), ("margin-64", 512, 1, 2048)):
        c = pl[name][1][0]
        h = 0.5 * (b[i0 + size - 1] - b[i0])
        gap = b[i0] - c - max(P.D_NEAR[r - 1], P.MARGIN * h)
        assert 0.0 < gap < 2e-5, (name, gap)
        fm = cases[name].geometry(P.RUN["default"]).node_form(i0 // 64, 0)
        assert fm is not None and fm[1:4] == (size, nc_of[(size, r)], r), (name, fm)
    for at in P.CLUSTER_AT:
        c = cases[f"cluster-{at}"]
        assert len(c.table.nu) == P.CLUSTER and c.real == [at] and len(c.ghosts) == P.CLUSTER - 1
        assert np.all(np.diff(c.table.nu) > 0) and c.table.nu[-1] - c.table.nu[0] < c.nu[1] - c.nu[0]
    temps, cold_thick = set(), False
    for name in cases.names():
        c = cases[name]
        assert c.K in P.K_SETS and min(p for _, p in c.states) >= P.P_LO and max(p for _, p in c.states) <= P.P_HI * (1 + 1e-12)
        temps |= {c.states[k][0] for k in c.ksel}
        cold_thick |= any(c.states[k][0] < 143.6 and c.states[k][1] > 1e5 for k in c.ksel)
    assert temps == set(P.T_SET) and cold_thick
    assert {cases[n].K for n in cases.names()} == set(P.K_SETS)


def test_probes_isolated_capped_and_above_underflow(cs, cases):
    """every probe sees exactly one line; at most MAX_PROBES per case; with S = 1e-20 and cut <= 500 no 40-digit value is of the underflow
    class (none is skipped from a comparison); the ghosts' sum stays below 1e-100 of the line's term; the Voigt gas of col/second reaches no
    point of the grid"""
    n = 0
    for name in cases.names():
        c = cases[name].reference()
        assert 0 < len(c.pr) <= P.MAX_PROBES, (name, len(c.pr))
        assert c.isolation() == [], name
        live = c.want[~c.zero]
        assert live.size and np.all(live >= 1e-60) and R.split(live)[1] == 0.0, name
        assert np.array_equal(c.zero, np.abs(c.nu[c.i] - [c.centre(k, l) for k, _, l in c.pr]) > c.cut), name
        if c.ghosts:
            worst = max(float(R.sigma_isolated(3, c.lines[0][0]["nu"], c.lines[0][0], *c.states[k], P.CONC * c.states[k][1], c.cut)[0]) for k in c.ksel) / float(np.min(live))
            assert (P.CLUSTER - 1) * P.GHOST_RATIO * worst < 1e-100, (name, worst)
        n += len(c.pr)
    v = cases["col/second"].tables[0]
    assert len(v.nu) == 1 and v.nu[0] + 25.0 < cases.grids["base"][0] and len(cases["col/graph"].tables) == 1
    print(f"{n} probes in {len(cases.names())} cases")


def test_crossing_probes_straddle(cases):
    """the two probes on either side of 3, 30, 120 cm^-1, the cut-off, the s crossings and the state's dQ lie on the two sides"""
    n = 0
    for name in cases.names():
        c = cases[name]
        have = set(c.pr)
        for (k, l), named in c.cross.items():
            cen = c.centre(k, l)
            for kind, thr, d in named:
                for sg in (-1.0, 1.0):
                    idx = P.I._near(c.nu, cen + sg * d)
                    assert all((k, i, l) in have or abs(c.nu[i] - cen) > c.cut for i in idx)
                    if len(idx) == 2 and (c.nu[idx[0]] - cen) * (c.nu[idx[1]] - cen) > 0.0:
                        lo, hi = sorted(abs(c.nu[i] - cen) for i in idx)
                        assert lo <= d <= hi, (name, k, l, kind, thr)
                        n += 1
    assert n > 400
    print(f"{n} crossings straddled")


def test_every_form_is_reached(cases):
    """every evaluation form of the fast path, and the generic kernel, is reached by at least one probe with a non-zero 40-digit value
    under the runs the device test compares; the node forms are those of the base grid's plans under the four node settings"""
    b = cases.grids["base"]
    plans = [P.levels(b, 500.0, True, r.force64)[1] for r in P.RUNS if r.interp]
    want = P.forms_wanted(plans)
    seen = {}
    for name in cases.names():
        c = cases[name].reference()
        for run in cases.runs(name):
            for strict in (True, False):
                for q, fm in enumerate(c.forms(run, strict)):
                    if not c.zero[q]:
                        seen.setdefault(fm, f"{name} {run.name}")
    for fm in sorted(want, key=str):
        print(fm, "first reached in", seen.get(fm))
    missing = sorted(want - set(seen), key=str)
    assert not missing, missing
    assert len(want) >= 150


def _names():
    import clearsky_jl_amd
    return P.Cases(clearsky_jl_amd).names()


@pytest.mark.parametrize("name", _names())
def test_oracle_meets_both_bounds(cs, O, cases, name):
    """O.shape_bang("PHCO2") at the device's probes of every case: within the hard bound with C0_ORACLE everywhere and, at s >= 1e3, within
    the sharp bound of the scalar form -- the reference and the model are right before the device meets them"""
    c = cases[name].reference()
    pts = np.unique(c.i)
    col = np.searchsorted(pts, c.i)
    got = np.zeros(len(c.pr))
    for k in c.ksel:
        T, Pk = c.states[k]
        s = O.shape_bang("PHCO2", c.nu[pts], c.table, T, Pk, P.CONC * Pk, c.cut, strict_ends=False)
        m = c.k == k
        got[m] = s[col[m]] * (P.CONC if c.lines[0][1] is not None else 1.0)
    wh, ws, per = P.compare(c, got, P.SCALAR, name, c0=R.C0_ORACLE, scalar=True, strict=False)
    print(f"{name}: {len(c.pr)} probes, oracle error / bound  hard {wh:.3f}  sharp {ws:.3f}")
