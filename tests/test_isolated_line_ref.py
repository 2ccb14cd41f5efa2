"""Host tests of tests/isolated_line_ref.py: what tests/test_gpu_isolated_line.py presupposes of its inputs, its probes and its two bounds is
checked here without a GPU -- every probe sees one line, no test holds more than MAX_PROBES, no probe is of the underflow class, the
crossing probes straddle their thresholds, the grids sit where the dispatch rules put them, and the oracle (oracle/cs_oracle.c: the
scalar form of the model) meets both bounds at the device's probes before the device is held to them."""
import math

import numpy as np
import pytest

import isolated_line_ref as I
import lineparam_ref as R


@pytest.fixture(scope="module")
def cases(cs, tmp_path_factory):
    d = tmp_path_factory.mktemp("isolated")
    return I.Cases(cs, R.shifted_table(cs, d), I.low_shifted_table(cs, d))


def test_grids_sit_on_the_rules(cs, cases):
    """the short grid: 40 tiles and a last tile of one point, three interval sizes; the four-level grid: four; the long grid: the
    smallest point count with tiles x ceil(K/16) >= 1024, intervals x ceil(K/16) >= 2048 and tiles x K >= 16384 at K = 61"""
    assert I.SHORT_N == 2561 and I.tiles(I.SHORT_N) == 41 and (I.SHORT_N - 1) % 64 == 0
    assert cases.plan(cases.short) == [512, 256, 128] and cases.plan(cases.low) == [512, 256, 128]
    assert I.FOUR_N == 8193 and cases.plan(cases.four) == [1024, 512, 256, 128]
    n = cases.n_long
    assert all(I.long_rules(n, cases.plan_of_n(n))) and not all(I.long_rules(n - 1, cases.plan_of_n(n - 1)))
    g = -(-I.NP_COL // 16)
    assert I.tiles(n) * g >= 1024 and I.n_itot(cases.plan_of_n(n), n) * g >= 2048 and I.tiles(n) * I.NP_COL >= 16384
    cen = I.long_centres(n)
    assert len(cen) >= 3 and np.all(np.diff(cen) > 2 * I.CUT) and cen[0] - I.CUT > cases.long[0] and cen[-1] + I.CUT < cases.long[-1]
    print(f"long grid: {n} points, plan {cases.plan_of_n(n)}, {len(cen)} lines")
    pl = I.placements()
    nu = cases.short
    assert pl["mid-tile"][0] == nu[20 * 64 + 32] and nu[1023] < pl["between-tiles-1024"][0] < nu[1024] and 1024 % 512 == 0
    assert pl["three-points-in"][0] == nu[3] and pl["outside-0.4cut"][0] == nu[0] - 10.0
    assert nu[0] < pl["edge-in-first-tile"][0] + I.CUT < nu[1] and pl["exactly-cut"][0] + I.CUT == nu[0]
    assert sorted({K for _, K in pl.values()} | {cases["batch/low-vvh"].K}) == [1, 16, 17, 33]
    assert I.LOW_CENTRE - I.CUT <= 0.0 and cases.low[0] + I.LOW_CENTRE <= I.CUT
    # the eight-tiles-per-wave grid: the smallest point count of the rule and one point more (a ragged last tile); two lines more than
    # 2 x cut apart, one two points into a tile that is the first of a wave's eight, one in the middle of the last complete tile
    c = cases["col/fine-rep8"]
    n = len(c.nu)
    assert I.rep_rules(n - 1, I.REP_LINES) and not I.rep_rules(n - 2, I.REP_LINES) and n % 64 not in (0, 1) and I.tiles(n) * I.NP_COL < 524288
    assert c.nu[0] == I.FINE_NU0 and abs((c.nu[-1] - c.nu[0]) / (n - 1) - I.FINE_DNU) < 1e-12 and len(c.lines) == I.REP_LINES
    ca, cb = (ln[0]["nu"] for ln in c.lines)
    assert cb - ca > 2 * I.CUT and I.REP_TILE % 8 == 0 and ca == c.nu[64 * I.REP_TILE + 2] and cb == c.nu[64 * (I.tiles(n) - 2) + 32]
    print(f"eight-tile grid: {n} points, {I.tiles(n)} tiles, lines at {ca:.4f} and {cb:.4f}")


def test_probes_isolated_capped_and_above_underflow(cs, cases):
    """every probe of every case sees exactly one line (none beyond the cut-off) and no other line's mirror term; at most MAX_PROBES per
    test; pressures all above 0, and the Lorentz wing at the cut-off, C S(T) gamma / (pi (cut^2 + gamma^2)), far above UNDERFLOW"""
    n = 0
    for name in cases.names():
        c = cases[name]
        assert 0 < len(c.pr) <= I.MAX_PROBES, (name, len(c.pr))
        assert c.isolation() == [], name
        assert min(P for _, P in c.states) >= I.P_LO > 0.0 and max(P for _, P in c.states) <= I.P_HI * (1 + 1e-12)
        for k, l in sorted({(k, l) for k, _, l in c.pr}):
            ln, C, frac, _ = c.lines[l]
            T, P = c.states[k]
            _, ga = R.widths(ln, T, P, frac * P)
            S = float(R.intensity(ln, T, (c.code & ~R.PSHIFT) in (5, 6, 7))[0])
            assert (C or 1.0) * S * ga / (math.pi * (c.cut ** 2 + ga ** 2)) > 1e-50 > 1e200 * R.UNDERFLOW, (name, k, l)
        n += len(c.pr)
    # the clusters: ghosts within one grid step above their line, GHOST_RATIO of its strength; with the profile's largest ratio inside the
    # cut-off, f(0) / f(cut) of the narrowest state, their sum stays below 1e-100 of the line's own term at every probe
    for name in cases.names():
        c = cases[name]
        assert bool(c.ghosts) == name.endswith("-cluster")
        if not c.ghosts:
            continue
        assert len(c.ghosts) == I.GHOSTS * len(c.lines) and len(c.ghosts) + len(c.lines) >= 64 and max(r for _, r in c.ghosts) <= I.GHOST_RATIO
        cen = np.array([ln[0]["nu"] for ln in c.lines])
        off = np.array([min(v - cen[cen <= v]) for v, _ in c.ghosts])
        assert np.all(off > 0.0) and np.max(off) < float(c.nu[1] - c.nu[0])
        worst = 0.0
        for k in c.ksel:
            al, ga = c.widths(k, 0)
            worst = max(worst, float(R.fvoigt(R._m(0.0), R._m(al), R._m(ga)) / R.fvoigt(R._m(c.cut), R._m(al), R._m(ga))))
        assert I.GHOSTS * I.GHOST_RATIO * worst < 1e-100, (name, worst)
    # the long grid deals every compared state to one of its lines; every other column case compares all eight in every line it probes
    dealt = sorted(k for k, _ in {(k, l) for k, _, l in cases["col/long"].pr})
    assert dealt == list(I.STATES_COMPARED) and sorted({k for k, _, _ in cases["col/long-cluster"].pr}) == dealt
    for name in cases.names():
        if name.startswith("col/") and "long" not in name:
            assert sorted({k for k, _, _ in cases[name].pr}) == list(I.STATES_COMPARED), name
    # widths: the narrowest states have series radii of a fraction of a cm^-1, the widest R4 beyond the cut-off
    c = cases["col/short"]
    w = [c.widths(k, 0) for k in range(c.K)]
    assert I.radius(3, *w[0]) < 1.0 and I.radius(4, *w[-1]) > I.CUT > I.radius(8, *w[-1])
    print(f"{n} probes in {len(cases.names())} cases")


def test_crossing_probes_straddle(cs, cases):
    """the two probes on either side of each distance where s crosses 100, 1e3, 1e4 and |d| crosses R8, R4, R3 (own widths, group's
    widest) really lie on the two sides: s and |d| / R_n recomputed at both"""
    n = 0
    for name in cases.names():
        c = cases[name]
        have = set(c.pr)
        for (k, l), named in c.cross.items():
            cen = c.centre(k, l)
            al, ga = c.widths(k, l)
            for kind, thr, d in named:
                for sg in (-1.0, 1.0):
                    idx = I._near(c.nu, cen + sg * d)
                    assert all((k, i, l) in have for i in idx)
                    if len(idx) < 2:
                        continue
                    off = [c.nu[i] - cen for i in idx]
                    dist = sorted(abs(x) for x in off)
                    if kind == "s":
                        lo, hi = (I.s_of(x, al, ga) / thr for x in dist)
                    else:
                        lo, hi = (x / d for x in dist)
                    if off[0] * off[1] < 0.0:   # the centre lies between the two points too: the one on the crossing's side is beyond it
                        x = abs(off[1] if sg > 0 else off[0])
                        assert (I.s_of(x, al, ga) / thr if kind == "s" else x / d) >= 1.0 - 1e-12, (name, k, l, kind, thr, x)
                    else:
                        assert lo <= 1.0 + 1e-12 and hi >= 1.0 - 1e-12, (name, k, l, kind, thr, lo, hi)
                    n += 1
    assert n > 1000
    print(f"{n} crossings straddled")


def test_rep8_core_probes(cs, cases):
    """col/fine-rep8, per line: at least as many probes in each tier of the near-line kernels (100 <= s < 1e3, s < 100) as
    test_gpu_isolated_line.py::test_coverage asks of col/fine (200); the cores of both lines cross the tile ends the case is about.
    One count cannot reach 200: the second line sits in the last complete tile so that its core runs into the ragged tile and off the
    grid, and the ring 100 <= s < 1e3 (30 to 90 points from the centre in the narrow states) has its upper half beyond the last point --
    wherever in that tile the centre is put, at most 170 such probes exist.  The lower half is whole, so half the figure is asked there."""
    c = cases["col/fine-rep8"].reference()
    m, _ = c.sharp(I.RunForm())
    line = np.array([l for _, _, l in c.pr])
    nt = I.tiles(len(c.nu))
    for l, tiles_met in ((0, (I.REP_TILE - 1, I.REP_TILE, I.REP_TILE + 1)), (1, (nt - 3, nt - 2, nt - 1))):
        core0, core1 = (int(np.sum(m & (line == l) & sel)) for sel in ((c.s >= 100.0) & (c.s < 1e3), c.s < 100.0))
        assert core1 >= 200 and core0 >= (200 if l == 0 else 100), (l, core0, core1)
        met = sorted({int(i) // 64 for i in c.i[m & (line == l) & (c.s < 1e3)]})
        assert set(tiles_met) <= set(met), (l, met)
        print(f"col/fine-rep8 line {l}: {core0} probes with 100 <= s < 1e3, {core1} with s < 100, in tiles {met}")


@pytest.mark.parametrize("name", ["batch/mid-tile", "batch/between-tiles-1024", "batch/low-vvh", "batch/fine", "col/fine-rep8", "col/low-lbl"])
def test_oracle_meets_both_bounds(cs, O, cases, name):
    """the oracle at the device's probes: within lineparam_bound(C0_ORACLE) everywhere, and within the sharp bound of the scalar form (no
    reciprocal terms: its divisions are IEEE; below s = 1e4 faddeeva_ref.bound(x, y, "scalar") per probe, the line core included) -- the
    reference and the model are right before the device meets them"""
    import test_lineparam_ref as TL
    c = cases[name].reference()
    sl = c.tables[0]
    pts = np.unique(c.i)
    col = np.searchsorted(pts, c.i)
    got = np.zeros(len(c.pr))
    for k in c.ksel:
        T, P = c.states[k]
        s = TL.oracle_sigma(cs, O, c.code, c.nu[pts], sl, T, P, I.CONC * P, c.cut)
        m = c.k == k
        got[m] = (c.lines[0][1] or 1.0) * s[col[m]]        # (a column case: the concentration is a factor of its values)
    hard = np.array([R.lineparam_bound(f, R.C0_ORACLE) for f in c.infos])
    worst_h = R.check(got, c.want, hard, c.zero, what=name + ", hard")
    m, b = c.sharp(I.RunForm(scalar=True, interp=False), c0=R.C0_ORACLE)
    worst_s = R.check(got[m], c.want[m], b[m], c.zero[m], what=name + ", sharp")
    assert R.split(c.want[~c.zero])[1] == 0.0          # the underflow class is empty
    assert np.array_equal(m, ~c.zero)                  # every probe with a term is under the sharp bound, the core included
    core = [int(np.sum(m & (c.s < 100.0))), int(np.sum(m & (c.s >= 100.0) & (c.s < 1e3))), int(np.sum(m & (c.s >= 1e3) & (c.s < 1e4)))]
    assert min(core) >= (100 if name in ("batch/fine", "col/fine-rep8") else 4 if name == "batch/mid-tile" else 0), core
    lo = c.s < 1e4
    worst_c = R.check(got[m & lo], c.want[m & lo], b[m & lo], c.zero[m & lo], what=name + ", sharp, s < 1e4")
    print(f"{name}: {len(c.pr)} probes ({int(m.sum())} sharp; s < 100: {core[0]}, < 1e3: {core[1]}, < 1e4: {core[2]}), oracle error / bound  hard {worst_h:.3f}  "
          f"sharp {worst_s:.3f} (s < 1e4: {worst_c:.3f}; bounds there {b[m & lo].min():.1e} .. {b[m & lo].max():.1e})")


def test_allowance_below_1e4(cs):
    """the Faddeeva allowance of the sharp bound is faddeeva_ref's per-probe bound below s = 1e4, of the branch that serves the probe; both
    branches count within S_EDGE of s = 100 and both grids within S_EDGE of the grid choice's boundary; from 1e3 on the six-term and the
    matrix forms count as before, and the far side of 1e4 is what it was"""
    import faddeeva_ref as FR
    dev, sca = I.RunForm(), I.RunForm(scalar=True)
    assert dev.allowance(3.0, 0.01) == FR.bound(3.0, 0.01, "device", "near") and sca.allowance(3.0, 0.01) == FR.bound(3.0, 0.01, "scalar", "near")
    assert dev.allowance(12.0, 0.5) == FR.bound(12.0, 0.5, "device", "mid") < 5e-14
    assert dev.allowance(6.0, 8.0) == max(FR.bound(6.0, 8.0, "device", "mid"), FR.bound(6.0, 8.0, "device", "near"))
    assert dev.allowance(0.125, 0.01) == max(FR.bound(0.125, 0.01, "device", "near-int"), FR.bound(0.125, 0.01, "device", "near-half"))
    x = math.sqrt(2e3)
    cap = I.MID + 2 * 4 * I.U
    assert dev.allowance(x, 0.1) == max(min(FR.bound(x, 0.1, "device", "mid"), cap), I.ALLOW["near6"] + I.rcp_fast(x * x + 0.01), I.ALLOW["matrix8"])
    assert sca.allowance(x, 0.1) == min(FR.bound(x, 0.1, "scalar", "mid"), cap) == cap and sca.allowance(30.0, 40.0) == FR.bound(30.0, 40.0, "scalar", "mid") < cap
    for xx, yy in ((x, 0.1), (30.0, 40.0), (60.0, 1e-3), (1.0, 99.0)):      # never above what the model took there before
        assert dev.allowance(xx, yy) <= dev.allowance_s(xx * xx + yy * yy) and sca.allowance(xx, yy) <= sca.allowance_s(xx * xx + yy * yy)
    for x in (125.0, 1000.0, 32768.0):
        assert dev.allowance(x, 0.0) == dev.allowance_s(x * x) and sca.allowance(x, 0.0) == sca.allowance_s(x * x)
    assert dev.allowance(5.0, 1.0, lorentz=True) == I.ALLOW["lorentz"]


def test_conditioning_term(cs, cases):
    """the conditioning term is 0 without interpolation and where the line is inside the probe's interval; elsewhere at least U x Lebesgue,
    and below U x Lebesgue x levels x ((2 + m) / m)^2 x 1.01 for a Lorentz-like wing at margin m"""
    c = cases["batch/between-tiles-1024"].reference()
    assert not np.any(c.conditioning(I.RunForm(interp=False)))
    for m in (0.3, 0.15):
        cd = c.conditioning(I.RunForm(margin=m))
        nz = cd > 0
        assert nz.any() and np.all(cd[nz] >= I.U * I.LEBESGUE) and np.max(cd) <= I.U * I.LEBESGUE * 3 * ((2 + m) / m) ** 2 * 1.01
        cen = c.centre(0, 0)
        assert not np.any(cd[np.abs(c.nu[c.i] - cen) < 64 * m * I.SHORT_DNU])   # (nearer than margin x the smallest half-width)
