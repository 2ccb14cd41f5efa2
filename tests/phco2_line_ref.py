"""PHCO2 (shape code 3) on isolated lines: tables, grids, placements, probe sets, the classification of a probe by the evaluation form that
serves it, and the error model -- shared by tests/test_phco2_line_ref.py (host) and tests/test_gpu_phco2_line.py (device).  The 40-digit
values are lineparam_ref.sigma_isolated(3, ...); nothing here reads the oracle or the GPU.

Inputs.  CO2 tables (lineparam_ref.table) whose lines lie more than 2 x cut apart, so that a probe is within the cut-off of at most one
line and the device's value there IS one line's term in one evaluation form.  "Cluster" tables hold CLUSTER = 130 lines GHOST_STEP apart,
one of them real and the others GHOST_RATIO = 1e-120 of its strength: the 16- and 32-node paths of k_phco2_nodes (ph_segment_lds) deal
line i of a 64-line batch to part i mod nparts and start a second batch after 64, so the real line at cluster index 0, 1, 2, 3, 63, 64, 65
sits in every part and in both batches.

The rules restated here from the sources (csrc/cs_kernels.h, csrc/cs_api.hip), as tests/test_gpu_dispatch.py restates its own:
  fast_ok        phco2_fast_ok: cut >= 130, the widest near zone inside 2.9 cm^-1, mean tile span <= 5, no tile wider than 27 cm^-1
  levels         ph_levels: sizes 8192 .. 128 (64 with key 10 bit 1), per region the node count 16 / 32 / 64 from (nc - 1) log10 rho >= 18, the
                 virtual levels in launch order and par[] (the next larger size that carries the region).  The host test holds it to
                 cs.phco2_plan on every grid used.  ph_levels' rule "D_far - max(D_near, margin h) - size dnu >= 5 % of the region" only
                 gets easier as the size shrinks, so a region carried at one size is carried at every smaller one: par[] never jumps a size
                 on any grid (asserted; the issue's "carried at one size and skipped at the next" can only mean the next LARGER size)
  tile_win       phwin_body: the six uniform sets, four boundary sets, the core [L1, R1) with [C0, C1), and E0 / E1
  itv_win        phiwin_body: the six region-uniform ranges of an interval
  zone_q         zone_compute: dQ and the 4-term range [Q0, Q1) of a (state, tile)
  node_two       k_phco2_nodes: two[r] from `need`
A probe's form (Geometry.form) follows from them and from the settings of the run alone -- it is never asked of the device:
  ("uniform", region, side, "two" | "four")      a tile's uniform set in k_phco2, by the zone bound
  ("pred", side)                                 the cut-off edge segments [W0, E0) and [E1, W1) of region 3 (predicate on)
  ("boundary", b, "near" | "far")                boundary set b = 0 .. 3 (120 left, 30 left, 30 right, 120 right), the lane's side of it
  ("core", "voigt")                              |d| < 3 in the inner Voigt pass (3 cm^-1 cut-off)
  ("core", "half", side)                         |d| > 3 for a line of [L1, C0) / [C1, R1): k_phco2's halves beside that pass
  ("core", "own", "near" | "far")                k_phco2's own loop (cs_set_tuning key 9), |d| < 3 or beyond
  ("node", size, nc, region, side, "low"|"high") an interval's own range at a virtual level: [lo, pa) below or [pb, hi) above the parent's
  ("generic",)                                   k_linesum<SH_PHCO2> (off the fast path)

The hard bound is lineparam_bound(C0_GPU) with code 3's chi term; where the fast path serves a probe beyond 3 cm^-1 the term is the
factorised form's: chi = exp(a_r -+ b_r (nu - nu_c)) x exp(+- b_r (nul - nu_c)), nu_c = (nu_1 + nu_N) / 2 (ph_grid), a_r as ph_coef
forms them (3 B1 | -27 B1 + 30 B2 | -27 B1 - 90 B2 + 120 B3): per coefficient B_q the multipliers of every product it enters add up
(fact_mult), times lineparam_ref.ph_coef_abs, plus 2 ulp per exponential (chi_rounding).

The sharp bound (probes with s = x^2 + (chi y)^2 >= 1e3) replaces the 2e-13 Faddeeva allowance by what the sources give for the form:
  far bodies (ph_term, both)      eps (series_radii.json) + 60 / s^4 below s = 1e6 (the 4-term body, isolated_line_ref) + rcp_fast(s) + 2 x 4 U.
                                  The 2-term body keeps EVERY u and u^2 term of the series (1 + 1.5 u + (3.75 - 2 y^2 - 15 t + 12 t^2) u^2, t =
                                  y^2 u): what it drops is u^3 p3(t), |p3| <= 13.125 on [0, 1], below 1.4e-17 for s >= far_s = 1e6 WHATEVER y
                                  is -- so chi > 1 (T < 143.6 K) cannot take it out of its budget: the zone bound only decides between two
                                  bodies that are both inside eps there.  (The "15 y^2 / s^3" of the Voigt path's mode-0 body is not dropped here.)
  core, inner Voigt pass          isolated_line_ref.RunForm().allowance_s(s): near6, the matrix forms, mid
  own core loop, k_linesum        fad_re: its far branch divides (IEEE), fad_mid below s = 1e4 (1e-14, cs_faddeeva.h:7): the scalar model;
                                  the own loop takes ph_term for lines no lane of the wave has inside s < 1e4, so the larger of both
  interpolated (node forms)       U x Lambda(nc) x max_I f / f(nu), Lambda(n) = (2 / pi) ln n + 1 the Lebesgue constant of the level's own node
                                  count, ONCE (no cascade: every level is carried to the grid by itself), plus the truncation ph_levels' rule
                                  promises, 1e-18 x max_I f / f(nu); max_I f from the 40-digit values at the interval's ends (both are probes;
                                  inside one region and side the term is monotone or has its largest value at an end: chi / d^2 with
                                  ln chi linear has no interior maximum)
The oracle is held to the scalar model (IEEE divisions, one exponential).

Recorded figures: see tests/test_gpu_phco2_line.py.
"""
import math

import numpy as np

import isolated_line_ref as I
import lineparam_ref as R
from clearsky_jl_amd import constants as C_

U = R.U
KC, KRGAS, KSQLN2, KTMAX, KTREF, KATM = 299792458.0, 8.31446262, 0.8325546111576977, 1000.0, C_.Tref, C_.atm      # cs_kernels.h:25-33
MARGIN, FAR_S = 0.3, 1e6                                           # kChebMargin (cs_kernels.h:567), cs_ctx::far_s
D_NEAR = (3.0, 30.0, 120.0)
CUTS = (500.0, 200.0, 100.0)
T_SET = (25.0, 100.0, 143.0, 144.0, 296.0, 1000.0)
K_SETS = (1, 5, 17)
P_LO, P_HI = 1.0, 3e6
CONC = 0.01
S_LINE = 1e-20
CLUSTER, GHOST_STEP, GHOST_RATIO = 130, 1e-5, 1e-120
CLUSTER_AT = (0, 1, 2, 3, 63, 64, 65)
MAX_PROBES = 2500
S_CROSS, S_SHARP = I.S_CROSS, I.S_SHARP
TRUNC_NODES = 1e-18                                                # ph_levels: (nc - 1) log10 rho >= 18


def lebesgue(n):
    return 2.0 / math.pi * math.log(n) + 1.0


# ---- grids --------------------------------------------------------------------------------------------------------------------------------

BASE_NU0, LOW_NU0, HIGH_NU0, BASE_DNU, BASE_N = 640.0, 320.0, 6400.0, 0.025, 64 * 100 + 17      # 101 tiles, the last of 17 points; about 160 cm^-1


def grids():
    """base: the uniform grid of the issue; low: the same below the cut-off (nu_1 - cut <= 0: zone_compute has no bound on y and runs the
    4-term body everywhere); geo: geometric, interval widths differ along it; short: fewer than 128 points (no levels); wide: tiles of
    32 cm^-1 > 27 (the k_linesum fallback); high: the base grid at 6400 cm^-1, where the Doppler width is ten times larger and 3 cm^-1 is
    only s = 3e4 at 1000 K -- region 1 needs the 4-term body there whatever the Lorentz width (two[r] of k_phco2_nodes false, dQ > 3)"""
    return {"base": I.grid(BASE_NU0, BASE_DNU, BASE_N), "low": I.grid(LOW_NU0, BASE_DNU, BASE_N), "geo": np.geomspace(600.0, 800.0, BASE_N),
            "short": np.linspace(700.0, 702.0, 90), "wide": np.linspace(100.0, 1300.0, 2400), "high": I.grid(HIGH_NU0, BASE_DNU, BASE_N)}


# ---- the rules, restated ---------------------------------------------------------------------------------------------------------------------

class Run:
    """the settings of one run: interp (cs_set_interp), tune {9: own core, 10: node counts / 64-point intervals}"""

    def __init__(self, name, interp=True, tune=None):
        self.name, self.interp, self.tune = name, interp, dict(tune or {})
        self.own_core, self.force64 = self.tune.get(9, 0), self.tune.get(10, 0)

    def context(self, cs):
        ctx = cs.Context(0)
        ctx.set_interp(self.interp)
        for k, v in self.tune.items():
            ctx.set_tuning(k, v)
        return ctx


RUNS = [Run("default"), Run("interp-off", interp=False), Run("own-core", tune={9: 1}), Run("nodes-64", tune={10: 1}),
        Run("tiles-as-intervals", tune={10: 2}), Run("tiles-as-intervals-64", tune={10: 3})]
RUN = {r.name: r for r in RUNS}
SCALAR = Run("scalar", interp=False)


def fast_ok(nu, cut, mu_min):
    """phco2_fast_ok (cs_api.hip)"""
    n = len(nu)
    if cut < 130.0 or n < 2 or not nu[-1] > nu[0]:
        return False
    amax = ((nu[-1] + cut) / KC) * math.sqrt(2.0 * KRGAS * KTMAX / mu_min)
    if 100.0 * amax / KSQLN2 * (1.0 + 1e-6) > 2.9:
        return False
    if (nu[-1] - nu[0]) / (n - 1) * 64.0 > 5.0:
        return False
    if not max(nu[min(i + 63, n - 1)] - nu[i] for i in range(0, n, 64)) <= 27.0:
        return False
    return not 0.0888 * (0.5 * (nu[-1] - nu[0]) + cut) > 600.0


def wide_reach(T, g, cut):
    """ph_wide_regions (cs_api.hip), per region: reach / limit of a state of temperature T and Lorentz bound g -- the zeros of x^2 + (chi
    y)^2, d = +-i gamma chi_r(d), reach G sin(min(|b_r| G, pi / 2)) towards the real axis, G = gamma max(e^(a_r), e^(a_r - 2 b_r D_far)); the
    limit is D_r / 10"""
    B1, B2, B3 = 0.0888 - 0.16 * math.exp(-0.0041 * T), 0.0526 * math.exp(-0.00152 * T), 0.0232
    a, b = (3.0 * B1, -27.0 * B1 + 30.0 * B2, -27.0 * B1 - 90.0 * B2 + 120.0 * B3), (B1, B2, B3)
    out = []
    for r in range(3):
        G = g * math.exp(max(a[r], a[r] - 2.0 * b[r] * (30.0, 120.0, cut)[r]))
        out.append(G * math.sin(min(abs(b[r]) * G, 1.5707963267948966)) / (0.1 * D_NEAR[r]))
    return out


def wide_regions(sts_gamma, cut):
    """the regions (1-based) a launch keeps out of the levels because one of its states [(T, Lorentz bound)] is too wide: wide_reach > 1"""
    return frozenset(r + 1 for T, g in sts_gamma for r, x in enumerate(wide_reach(T, g, cut)) if not x <= 1.0)


def levels(nu, cut, interp=True, force64=0, margin=MARGIN, smin=128, smax=2048, drop=frozenset()):
    """ph_levels (cs_api.hip): (sizes carried, largest first; virtual levels [(size, nc, regions (1-based), {region: parent size or None})] in
    launch order; fine {region: smallest size that carries it or None}); drop: wide_regions of the launch's states"""
    n = len(nu)
    none = ([], [], {1: None, 2: None, 3: None})
    if not interp or n < 128:
        return none
    dnu = (nu[-1] - nu[0]) / (n - 1)
    szmax = 8192 if smax >= 2048 else smax
    szmin = 64 if (smin <= 128 and force64 & 2) else smin
    Df = (30.0, 120.0, cut)
    need, sizes = {}, []
    for i in range(8):
        sz = 8192 >> i
        if not (szmin <= sz <= szmax and 2.3 * sz * dnu <= 1.5 * cut and sz // 2 <= n and sz * dnu > 1e-8 * abs(nu[-1])):
            continue
        h = 0.5 * max(nu[min(i0 + sz - 1, n - 1)] - nu[i0] for i0 in range(0, n, sz))
        nd = {}
        for r in range(3):
            dn = max(D_NEAR[r], margin * h)
            if r + 1 in drop:
                continue
            if not Df[r] - dn - sz * dnu >= 0.05 * (Df[r] - D_NEAR[r]):
                continue
            x0 = 1.0 + max(D_NEAR[r] / h, margin)
            lr = math.log10(x0 + math.sqrt(x0 * x0 - 1.0))
            nd[r + 1] = 64 if force64 & 1 else (16 if 15.0 * lr >= 18.0 else 32 if 31.0 * lr >= 18.0 else 64)
        if nd:
            need[sz] = nd
            sizes.append(sz)
    if not sizes:
        return none
    vl, last = [], {1: None, 2: None, 3: None}
    for sz in sizes:
        for nc in (64, 32, 16):
            regs = tuple(r for r in (1, 2, 3) if need[sz].get(r) == nc)
            if regs:
                vl.append((sz, nc, regs, {r: last[r] for r in regs}))
        for r in need[sz]:
            last[r] = sz
    assert len(vl) <= 16                     # (CS_MAX_ALEVEL: beyond it ph_levels doubles node counts -- not restated, not reached)
    return sizes, vl, last


def _tol(nu, cut):
    return 1e-9 * (max(abs(nu[0]), abs(nu[-1])) + cut + 1.0)       # line_sum_phco2: one value per grid


class Geometry:
    """the sets of every tile and interval of one (grid, sorted line positions, record range [J0, J1), cut-off, run); form(i, j, ...) names
    the form that serves line j at point i"""

    def __init__(self, nu, nul, cut, run, mu, J=None, drop=frozenset()):
        self.nu, self.nul, self.cut, self.run = np.asarray(nu, float), np.asarray(nul, float), float(cut), run
        self.n = len(self.nu)
        self.J0, self.J1 = J if J is not None else (0, len(self.nul))
        self.mu_min, self.mu_max = float(np.min(mu)), float(np.max(mu))
        self.fast = fast_ok(self.nu, self.cut, self.mu_min)
        self.tol = _tol(self.nu, self.cut)
        self.nu_c = 0.5 * (self.nu[0] + self.nu[-1])
        self.sizes, self.vl, self.fine = levels(self.nu, self.cut, run.interp, run.force64, drop=drop) if self.fast else ([], [], {})
        self._tw, self._iw, self._tc, self._zq = {}, {}, {}, {}

    def lower(self, v):
        return self.J0 + int(np.searchsorted(self.nul[self.J0:self.J1], v, "left"))

    def upper(self, v):
        return self.J0 + int(np.searchsorted(self.nul[self.J0:self.J1], v, "right"))

    def span(self, size, t):
        return float(self.nu[t * size]), float(self.nu[min(t * size + size - 1, self.n - 1)])

    def tile_win(self, t):
        """phwin_body"""
        if t not in self._tw:
            vlo, vhi = self.span(64, t)
            cut, tol, lo = self.cut, self.tol, self.lower
            w = dict(W0=lo(vlo - cut - tol), W1=lo(vhi + cut + tol), L3=lo(vlo - 120.0 - tol), L2a=lo(vhi - 120.0 + tol), L2=lo(vlo - 30.0 - tol),
                     L1a=lo(vhi - 30.0 + tol), L1=lo(vlo - 3.0 - tol), C0=lo(vhi - 3.0 + tol), C1=lo(vlo + 3.0 - tol), R1=lo(vhi + 3.0 + tol),
                     R1b=lo(vlo + 30.0 - tol), R2=lo(vhi + 30.0 + tol), R2b=lo(vlo + 120.0 - tol), R3=lo(vhi + 120.0 + tol))
            prev = "W0"
            for name in ("L3", "L2a", "L2", "L1a", "L1"):
                w[name] = max(w[name], w[prev])
                prev = name
            w["R1"] = max(w["R1"], w["L1"])
            prev = "R1"
            for name in ("R1b", "R2", "R2b", "R3", "W1"):
                w[name] = max(w[name], w[prev])
                prev = name
            w["C0"] = min(max(w["C0"], w["L1"]), w["R1"])
            w["C1"] = min(max(w["C1"], w["C0"]), w["R1"])
            w["E0"] = min(max(lo(vhi - cut + tol), w["W0"]), w["W1"])
            w["E1"] = min(max(lo(vlo + cut - tol), w["E0"]), w["W1"])
            self._tw[t] = w
        return self._tw[t]

    def itv_win(self, size, T):
        """phiwin_body: (a[6], b[6]) in line order r3 left, r2 left, r1 left, r1 right, r2 right, r3 right"""
        if (size, T) not in self._iw:
            vlo, vhi = self.span(size, T)
            cut, tol = self.cut, self.tol
            dZ = MARGIN * 0.5 * (vhi - vlo)
            d1, d2, d3 = max(3.0, dZ), max(30.0, dZ), max(120.0, dZ)
            sv = (vhi - cut + tol, vlo - d3 - tol, vhi - 120.0 + tol, vlo - d2 - tol, vhi - 30.0 + tol, vlo - d1 - tol,
                  vhi + d1 + tol, vlo + 30.0 - tol, vhi + d2 + tol, vlo + 120.0 - tol, vhi + d3 + tol, vlo + cut - tol)
            lo = [self.lower(v) for v in sv]
            a = [lo[2 * s] for s in range(6)]
            b = [max(lo[2 * s + 1], lo[2 * s]) for s in range(6)]
            for s in range(1, 6):
                a[s] = max(a[s], b[s - 1])
                b[s] = max(b[s], a[s])
            self._iw[(size, T)] = (a, b)
        return self._iw[(size, T)]

    def zone_q(self, t, T, gbound):
        """zone_compute: (Q0, Q1) of the state on tile t -- the 4-term range of k_phco2's uniform sets; (None, None): everywhere"""
        vlo, vhi = self.span(64, t)
        w = self.tile_win(t)
        vth = math.sqrt(2.0 * KRGAS * T)
        amax = ((vhi + self.cut) / KC) * vth / math.sqrt(self.mu_min)
        dA = 100.0 * amax / KSQLN2 * (1.0 + 1e-6)
        dAA = dA * math.sqrt(FAR_S * 1e-4)
        vmin, y2b = vlo - self.cut, 1e300
        if vmin > 0.0 and w["W1"] > w["W0"]:
            amin = (max(vmin, self.nul[w["W0"]]) / KC) * vth / math.sqrt(self.mu_max)
            y2b = (gbound * KSQLN2 / amin) ** 2
        if y2b >= 1e290:
            return None, None, dAA
        dQ = dA * math.sqrt(max((1.5e16 * y2b) ** (1.0 / 3.0), FAR_S) * 1e-4) if y2b > 60.0 else dAA
        return self.lower(vlo - dQ), self.upper(vhi + dQ), dQ

    def node_two(self, size, T, region, Tk, gbound):
        """k_phco2_nodes: two[r] of the state on interval T of `size` (the interval's ends stand for its outermost nodes)"""
        vlo, vhi = self.span(size, T)
        a, b = self.itv_win(size, T)
        vth = math.sqrt(2.0 * KRGAS * Tk)
        amax = ((vhi + self.cut) / KC) * vth / math.sqrt(self.mu_min)
        vmin = max(vlo - self.cut, self.nul[a[0]]) if b[5] > a[0] else vlo - self.cut
        need = 1e300
        if vmin > 0.0:
            yb = gbound * KSQLN2 / ((vmin / KC) * vth / math.sqrt(self.mu_max))
            need = max((1.5e16 * yb * yb) ** (1.0 / 3.0), FAR_S) * (1.0 + 1e-6)
        return (D_NEAR[region - 1] * KSQLN2 / amax) ** 2 >= need

    def node_form(self, t, j):
        """the virtual level whose own range holds line j for the intervals of tile t: ("node", size, nc, region, side, piece) or None"""
        i = 64 * t
        for size, nc, regs, par in self.vl:
            a, b = self.itv_win(size, i // size)
            for q in range(6):
                r = 3 - q if q < 3 else q - 2
                if r in regs and a[q] <= j < b[q]:
                    piece = "low"
                    if par[r] is not None:
                        pa_, pb_ = self.itv_win(par[r], i // par[r])
                        pa = min(max(pa_[q], a[q]), b[q])
                        pb = min(max(pb_[q], pa), b[q])
                        if pa <= j < pb:
                            continue                     # (the parent's: a larger level has named it already -- nesting)
                        piece = "low" if j < pa else "high"
                    return ("node", size, nc, r, "left" if q < 3 else "right", piece)
        return None

    def tile_class(self, t, j):
        """what serves line j on tile t, as far as the tile alone decides it (kept per (t, j))"""
        key = (t, j)
        if key in self._tc:
            return self._tc[key]
        w = self.tile_win(t)
        out = None
        if not w["W0"] <= j < w["W1"]:
            out = ("none",)                              # (beyond the cut-off of the whole tile)
        if out is None:
            out = self.node_form(t, j)
        if out is None:
            sets = (("W0", "L3"), ("L2a", "L2"), ("L1a", "L1"), ("R1", "R1b"), ("R2", "R2b"), ("R3", "W1"))
            for q, (lo, hi) in enumerate(sets):
                if w[lo] <= j < w[hi]:
                    out = ("pred",) if (q == 0 and j < w["E0"]) or (q == 5 and j >= w["E1"]) else ("uniform", 3 - q if q < 3 else q - 2)
        if out is None:
            for b, (lo, hi, D) in enumerate((("L3", "L2a", 120.0), ("L2", "L1a", 30.0), ("R1b", "R2", 30.0), ("R2b", "R3", 120.0))):
                if w[lo] <= j < w[hi]:
                    out = ("boundary", b, D)
        if out is None:
            assert w["L1"] <= j < w["R1"], (t, j, w)
            out = ("core", w["C0"] <= j < w["C1"])
        self._tc[key] = out
        return out

    def form(self, i, j, T, gbound, s):
        """the form that serves line j (index into nul) at point i in a state of temperature T, Lorentz bound gbound, s at the probe"""
        if not self.J0 <= j < self.J1:
            return ("none",)
        if not self.fast:
            return ("generic",)
        d = self.nu[i] - self.nul[j]
        side = "left" if d > 0.0 else "right"
        c = self.tile_class(i // 64, j)
        if c[0] in ("none", "node"):
            return c
        if c[0] == "pred":
            return ("pred", side)
        if c[0] == "uniform":
            zk = (i // 64, T, gbound)
            if zk not in self._zq:
                self._zq[zk] = self.zone_q(*zk)
            Q0, Q1, _ = self._zq[zk]
            return ("uniform", c[1], side, "four" if Q0 is None or Q0 <= j < Q1 else "two")
        if c[0] == "boundary":
            return ("boundary", c[1], "near" if abs(d) < c[2] else "far")
        if self.run.own_core:
            return ("core", "own", "near" if abs(d) < 3.0 else "far")
        if abs(d) > 3.0 and not c[1]:
            return ("core", "half", side)
        return ("core", "voigt")


def forms_wanted(plans):
    """every form of the issue's list; the node forms from the plans (levels()[1]) of the runs compared: a level without a parent has one
    piece"""
    out = {("uniform", r, sd, body) for r in (1, 2, 3) for sd in ("left", "right") for body in ("two", "four")}
    out |= {("boundary", b, sd) for b in range(4) for sd in ("near", "far")}
    out |= {("core", "voigt"), ("core", "own", "near"), ("core", "own", "far"), ("core", "half", "left"), ("core", "half", "right")}
    out |= {("pred", "left"), ("pred", "right"), ("generic",)}
    for vl in plans:
        for size, nc, regs, par in vl:
            out |= {("node", size, nc, r, sd, pc) for r in regs for sd in ("left", "right") for pc in (("low", "high") if par[r] else ("low",))}
    return out


# ---- the error model ----------------------------------------------------------------------------------------------------------------------------

def fact_mult(region, dc, dl):
    """per coefficient (B1, B2, B3): the sum of the multipliers of every product it enters in the factorised chi of `region` -- a_r (ph_coef),
    b_r |nu - nu_c| and b_r |nul - nu_c|"""
    m = [0.0, 0.0, 0.0]
    for q, x in enumerate(((3.0,), (27.0, 30.0), (27.0, 90.0, 120.0))[region - 1]):
        m[q] += x
    m[region - 1] += abs(dc) + abs(dl)
    return m


def chi_term(info, form, dc, dl):
    """what replaces info["chi_rnd"] for the form: the factorised chi's where the fast path evaluates chi beyond 3 cm^-1, the scalar one in
    k_linesum (and the oracle), 0 where chi = 1"""
    if info["region"] == 0:
        return 0.0
    if form[0] in ("generic", "none"):
        return info["chi_rnd"]
    return R.chi_rounding(fact_mult(info["region"], dc, dl), info["chi_abs"], 2)


_VOIGT = I.RunForm()


def allowance(form, s, scalar=False):
    """the sharp bound's replacement of the Faddeeva allowance (module docstring)"""
    t4 = I.trunc4(s)
    scal = (I.EPS + t4 if s >= 1e4 else I.MID) + 2 * 4 * U
    if scalar or form[0] == "generic":
        return scal
    vec = I.EPS + t4 + I.rcp_fast(s) + 2 * 4 * U
    if form[:2] == ("core", "voigt"):
        return _VOIGT.allowance_s(s)
    if form[:2] == ("core", "own"):
        return max(scal, vec)
    return vec


# ---- tables, states ----------------------------------------------------------------------------------------------------------------------------

def line_table(cs, centres, cluster_at=None):
    """one CO2 line per centre (isolated_line_ref.one_line_table's parameters); cluster_at: each centre starts a cluster of CLUSTER lines
    GHOST_STEP apart whose line `cluster_at` is the real one (moved so that IT sits at the centre)"""
    centres = np.atleast_1d(np.asarray(centres, float))
    if cluster_at is None:
        return I.one_line_table(cs, centres, S=S_LINE)
    nu = np.concatenate([c + GHOST_STEP * (np.arange(CLUSTER) - cluster_at) for c in centres])
    S = np.tile([S_LINE if q == cluster_at else S_LINE * GHOST_RATIO for q in range(CLUSTER)], len(centres))
    nu[cluster_at::CLUSTER] = centres
    return R.table(cs, 2, [1] * len(nu), nu, S, 0.07, 0.09, 300.0, 0.7)


GAMMA_AIR, GAMMA_SELF, N_AIR = 0.07, 0.09, 0.7            # isolated_line_ref.one_line_table


def gamma_of(T, P):
    """the Lorentz width of the tables' lines at (T, P), Pp = CONC P, in doubles"""
    return (KTREF / T) ** N_AIR * (GAMMA_AIR * (P - CONC * P) + GAMMA_SELF * CONC * P) / KATM


def pressure_at_reach(T, region, x, cut=500.0):
    """the pressure at which a state of temperature T has wide_reach x in `region` (bisection; the reach grows with the width)"""
    lo, hi = P_LO, P_HI
    assert wide_reach(T, gamma_of(T, lo), cut)[region - 1] < x < wide_reach(T, gamma_of(T, hi), cut)[region - 1]
    for _ in range(200):
        mid = math.sqrt(lo * hi)
        lo, hi = (mid, hi) if wide_reach(T, gamma_of(T, mid), cut)[region - 1] < x else (lo, mid)
    return lo


def states(K, seed=0):
    """K states: pressures log-spaced over 1 .. 3e6 Pa (K = 1: 1e5 Pa), the six temperatures of T_SET in turn from `seed` on.  seed =
    "calm": the temperatures rise with the pressure instead (K = 1: 296 K), so that no state is wide (wide_regions: nothing kept out of the
    levels).  seed = ("edge", T, region, x): the calm set with its last state but one replaced by one at temperature T whose wide_reach in
    `region` is x -- just under (or over) the limit of ph_wide_regions"""
    P = [1e5] if K == 1 else list(np.exp(np.linspace(math.log(P_LO), math.log(P_HI), K)))
    if seed == "calm" or isinstance(seed, tuple):
        out = [(T_SET[4] if K == 1 else T_SET[k * 6 // K], float(p)) for k, p in enumerate(P)]
        if isinstance(seed, tuple):
            _, T, region, x = seed
            out[K - 2] = (T, pressure_at_reach(T, region, x))
        return out
    return [(T_SET[(k + seed) % 6], float(p)) for k, p in enumerate(P)]


def compared(K):
    """the states compared of a call of K (the 40-digit values set the tests' time): the first, the last of the first block of four and the
    last of all (alone in its block in k_phco2_nodes, next to the padding to Kpad); of 17 also two from the middle"""
    return [0] if K == 1 else [0, 3, 4] if K == 5 else [0, 7, 12, 15, 16]


def column_states(cs, K=17, seed=2):
    """(P levels, T levels, [(T, P)] of the node states) of a K-level column with nlob = 2 (the nodes are the levels)"""
    sts = states(K, seed)
    P, T = np.array([p for _, p in sts]), np.array([t for t, _ in sts])
    Tn, _ = cs.lobattoevaluations(P, cs.formprofile(P, T), cs.formprofile(P, 0.029), 2)
    return P, T, list(zip(cs.nodevalues(Tn, 2), cs.nodepressures(P, 2)))


# ---- probes -----------------------------------------------------------------------------------------------------------------------------------

def _at(nu, v):
    return min(max(int(np.searchsorted(nu, v)), 0), len(nu) - 1)


def probe_indices(nu, c, sizes, cut, crossings):
    """grid indices of the probes of one (line, state) -- isolated_line_ref.probe_indices for any grid: +-12 points about the centre, both
    sides of every distance of `crossings`, first and last point of every tile and interval inside the cut-off, the last point inside and
    the first outside it, 32 log-spaced distances per side, the grid's ends"""
    n = len(nu)
    inside = np.nonzero(np.abs(nu - c) <= cut)[0]
    out = {0, n - 1}
    ic = _at(nu, c)
    out.update(i for i in range(ic - 12, ic + 13) if 0 <= i < n)
    for d in crossings:
        for sg in (-1.0, 1.0):
            out.update(I._near(nu, c + sg * d))
    if inside.size:
        a, b = int(inside[0]), int(inside[-1])
        out.update(i for i in (a - 1, a, b, b + 1) if 0 <= i < n)
        for size in sorted({64} | set(sizes)):
            for t in range(a // size, b // size + 1):
                out.update(i for i in (t * size, min(t * size + size - 1, n - 1)) if a <= i <= b)
        h = float(np.min(np.diff(nu)))
        for d in np.exp(np.linspace(math.log(h), math.log(cut), 32)):
            for sg in (-1.0, 1.0):
                if nu[0] <= c + sg * d <= nu[-1]:
                    i = _at(nu, c + sg * d)
                    out.add(i if i == 0 or abs(nu[i] - c - sg * d) < abs(nu[i - 1] - c - sg * d) else i - 1)
    return sorted(out)


class Case(I.Case):
    """isolated_line_ref.Case for code 3: its own probes, classification and bounds.  `real`: the index in its table of each real line"""

    def __init__(self, cs, name, nu, tables, sts, cut=500.0, concs=None, ksel=None, points_only=False):
        self.name, self.points_only = name, points_only
        super().__init__(cs, nu, levels(nu, cut)[0], tables, sts, code=3, cut=cut, concs=concs, ksel=ksel)

    def _build(self):
        self.table = self.tables[-1]                      # (the PHCO2 gas: the last of the case's tables)
        self.lines = [ln for ln in self.lines if ln[3] == len(self.tables) - 1]
        self.real = [int(np.argmin(np.abs(self.table.nu - ln[0]["nu"]) + (self.table.S < 1e-60))) for ln in self.lines]
        assert all(self.table.nu[j] == ln[0]["nu"] and self.table.S[j] == S_LINE for j, ln in zip(self.real, self.lines))
        pr, self.cross = [], {}
        for l in range(len(self.lines)):
            for k in self.ksel:
                al, ga = self.widths(k, l)
                named = [("D", D, D) for D in D_NEAR + (self.cut,)]
                for S in S_CROSS:
                    d2 = S * al * al / math.log(2.0) - ga * ga
                    if d2 > 0.0:
                        named.append(("s", S, math.sqrt(d2)))
                named.append(("dQ", 0.0, self.dq(k, l)))
                named = [c for c in named if c[2] <= self.cut]
                self.cross[(k, l)] = named
                pr += [(k, i, l) for i in probe_indices(self.nu, self.centre(k, l), self.sizes, self.cut, [c[2] for c in named])]
        reach = lambda k, i, l: abs(self.nu[i] - self.centre(k, l)) <= self.cut
        others = lambda k, i, l: any(reach(k, i, m) for m in range(len(self.lines)) if m != l)
        self.pr = sorted(p for p in set(pr) if reach(*p) or not others(*p))
        self.k = np.array([p[0] for p in self.pr])
        self.i = np.array([p[1] for p in self.pr])

    def gbound(self, k):
        """gamma_bound (cs_api.hip) for the case's table: every line has the same widths, so it is the line's own Lorentz width"""
        T, P = self.states[k]
        sl, frac = self.table, self.lines[0][2]
        r = KTREF / T
        f = max(r ** float(np.min(sl.na)), r ** float(np.max(sl.na)))
        return f * (abs(float(np.max(sl.gamma_a)) * (P - frac * P)) + abs(float(np.max(sl.gamma_s)) * frac * P)) / KATM * (1.0 + 1e-12)

    def dq(self, k, l):
        """the state's dQ (zone_compute) on the tile of the line's centre (the nearest tile for a line outside the grid)"""
        g = self.geometry(SCALAR)
        return g.zone_q(_at(self.nu, self.centre(k, l)) // 64, self.states[k][0], self.gbound(k))[2]

    def geometry(self, run, strict=True):
        """the Geometry of a run; strict: the record range of the vector methods (included_range: lines strictly inside nu_1 - cut, nu_N + cut)"""
        key = (run.name, strict)
        self._geo = getattr(self, "_geo", {})
        if key not in self._geo:
            nul = np.asarray(self.table.nu, float)
            J = (int(np.searchsorted(nul, self.nu[0] - self.cut, "right")), int(np.searchsorted(nul, self.nu[-1] + self.cut, "left"))) if strict else None
            drop = wide_regions([(self.states[k][0], self.gbound(k)) for k in range(self.K)], self.cut)      # (every state of the call)
            self._geo[key] = Geometry(self.nu, nul, self.cut, run, self.table.mu, J, drop)
        return self._geo[key]

    def forms(self, run, strict=True):
        """the form of every probe under the run"""
        self.reference()
        g = self.geometry(run, strict)
        return [g.form(i, self.real[l], self.states[k][0], self.gbound(k), self.s[q]) for q, (k, i, l) in enumerate(self.pr)]

    def reference(self):
        if hasattr(self, "want"):
            return self
        super().reference()
        for q, f in enumerate(self.infos):                 # s with the scaled Lorentz width
            d = self.nu[self.i[q]] - self.centre(self.k[q], self.pr[q][2])
            self.s[q] = I.s_of(d, f["alpha"], f["chi"] * f["gamma"])
        return self

    def bounds(self, run, c0=R.C0_GPU, scalar=False, strict=True):
        """(hard[len(pr)], sharp mask, sharp[len(pr)], forms) of a run: module docstring"""
        self.reference()
        key = (run.name, c0, scalar, strict)
        self._bnd = getattr(self, "_bnd", {})
        if key in self._bnd:
            return self._bnd[key]
        forms = self.forms(run, strict)
        g = self.geometry(run, strict)
        n = len(self.pr)
        hard, sharp = np.zeros(n), np.zeros(n)
        for q, (f, fm) in enumerate(zip(self.infos, forms)):
            nul = self.lines[self.pr[q][2]][0]["nu"]
            chi = f["chi_rnd"] if scalar else chi_term(f, fm, self.nu[self.i[q]] - g.nu_c, nul - g.nu_c)
            rnd = U * (c0 + R.model_terms(f) - f["chi_rnd"] + chi)
            hard[q] = rnd + R.FADDEEVA
            cond = 0.0
            if fm[0] == "node" and not self.zero[q] and self.want[q] >= R.UNDERFLOW:
                size, nc = fm[1], fm[2]
                a, b = (self.i[q] // size) * size, min((self.i[q] // size) * size + size - 1, len(self.nu) - 1)
                ends = [self._at[(self.k[q], e, self.pr[q][2])] for e in (a, b)]      # (interval ends inside the cut-off are probes)
                big = max(self.want[ends[0]], self.want[ends[1]], self.want[q]) / self.want[q]
                cond = (U * lebesgue(nc) + TRUNC_NODES) * big
            sharp[q] = rnd + allowance(fm, self.s[q], scalar) + cond
        self._bnd[key] = (hard, ~self.zero & (self.s >= S_SHARP), sharp, forms)
        return self._bnd[key]


def compare(case, got, run, what, c0=R.C0_GPU, scalar=False, strict=True):
    """got[len(case.pr)] against the reference under both bounds; returns (worst / hard, worst / sharp, {form: (worst / hard, worst / sharp)})"""
    got = np.asarray(got, float)
    hard, m, sharp, forms = case.bounds(run, c0, scalar, strict)
    every = np.ones(len(got), bool)
    wh = I._held(case, got, hard, every, what + ", hard")
    ws = I._held(case, got, sharp, m, what + ", sharp")
    live = ~case.zero & (np.abs(case.want) >= R.UNDERFLOW)
    err = np.where(live, np.abs(got - case.want) / np.where(live, np.abs(case.want), 1.0), 0.0)
    per = {}
    for q, fm in enumerate(forms):
        if live[q]:
            a, b = per.get(fm, (0.0, 0.0))
            per[fm] = (max(a, err[q] / hard[q]), max(b, err[q] / sharp[q] if m[q] else 0.0))
    return wh, ws, per


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------

def placements(g):
    """name -> (grid, centres, K, seed of the temperatures, cut-off, cluster index or None, runs compared).  Built from the rules of
    phwin_body / phiwin_body on the base grid: tile t spans nu[64 t] .. nu[64 t + 63], interval T of `size` nu[size T] .. ; a region-r set of
    an interval stays max(D_r, margin x half-width) away from it"""
    b, low = g["base"], g["low"]
    every = [r.name for r in RUNS]
    few = ["default", "interp-off"]
    eps = 1e-5
    h = lambda size: 0.5 * (size - 1) * BASE_DNU
    out = {
        # inside the grid: every boundary set with 3 and 30 cm^-1 on both sides, the core and its halves
        "mid-tile": ("base", [float(b[50 * 64 + 32])], 17, "calm", 500.0, None, every),      # (every region interpolated at K = 17)
        "tile-edge-4096": ("base", [float(b[4096])], 5, 1, 500.0, None, every),        # first point of a tile and of an interval of every size
        # 120 cm^-1 crossing a tile on either side needs the line near an end
        "near-lo": ("base", [float(b[400]) + 0.011], 5, 2, 500.0, None, every),
        "near-hi": ("base", [float(b[-400]) - 0.011], 5, 3, 500.0, None, every),
        # outside: whole tiles in regions 1, 2, 3 on each side
        "outside-lo-10": ("base", [BASE_NU0 - 10.0], 5, 4, 500.0, None, every),
        "outside-hi-10": ("base", [float(b[-1]) + 10.0], 5, 5, 500.0, None, every),
        "outside-lo-200": ("base", [BASE_NU0 - 200.0], 1, 0, 500.0, None, every),          # region 3 for the whole grid: the largest interval's set
        "outside-hi-200": ("base", [float(b[-1]) + 200.0], 1, 4, 500.0, None, every),
        # the cut-off edge crossing a tile (E0 / E1, the PRED segments); 270 lies inside [nu(4095) - cut, nu_N - cut): own range of the first
        # 4096-point interval below its parent's
        "edge-lo": ("base", [BASE_NU0 - 370.0], 5, 0, 500.0, None, every),
        "edge-hi": ("base", [float(b[-1]) + 370.0], 5, 3, 500.0, None, every),
        "exactly-cut-lo": ("base", [BASE_NU0 - 500.0], 1, 4, 500.0, None, ["default"]),
        # a grid point at exactly 3, 30, 120 cm^-1: centre = nu[i] -+ D is exact (same binade), so is nu[i] - centre
        "exact-3-left": ("base", [float(b[3000]) - 3.0], 1, 4, 500.0, None, few),
        "exact-3-right": ("base", [float(b[3000]) + 3.0], 1, 0, 500.0, None, few),
        "exact-30-left": ("base", [float(b[3000]) - 30.0], 1, 2, 500.0, None, few),
        "exact-30-right": ("base", [float(b[3000]) + 30.0], 1, 3, 500.0, None, few),
        "exact-120-left": ("base", [float(b[5500]) - 120.0], 1, 1, 500.0, None, few),
        "exact-120-right": ("base", [float(b[900]) + 120.0], 1, 5, 500.0, None, few),
        # just beyond max(D_r, margin h) below an interval's first point: the closest a set may come -- region 3 of a 1024-point interval
        # (16 nodes; the one from nu[3072], whose 2048-point parent reaches below it and so cannot hold the line), region 2 of a 2048-point
        # one (32), region 1 of a 512-point one (64: margin h = 1.9 < 3)
        "margin-16": ("base", [float(b[3072]) - 120.0 - eps], 5, 1, 500.0, None, few),
        "margin-32": ("base", [float(b[2048]) - max(30.0, MARGIN * h(2048)) - eps], 5, 0, 500.0, None, few),
        "margin-64": ("base", [float(b[2048]) - max(3.0, MARGIN * h(512)) - eps], 5, 1, 500.0, None, few),
        # ... and the same line with a 25 K, 3e6 Pa state in the call: gamma = 12 cm^-1 and chi up to 4.5 put a zero of x^2 + (chi y)^2 over
        # that interval, where 32 nodes left 4.9e-12 -- ph_wide_regions now keeps regions 1 and 2 of such a call out of the levels
        # ... and at the limit of that rule: a 25 K state at 0.95 of the region-2 limit in the 32-node position (region 1 is out, region 2
        # interpolated), one at 0.95 of the region-1 limit in the 64-node position (both interpolated), and one just over the region-2 limit
        "margin-32-edge": ("base", [float(b[2048]) - max(30.0, MARGIN * h(2048)) - eps], 5, ("edge", 25.0, 2, 0.95), 500.0, None, few),
        "margin-64-edge": ("base", [float(b[2048]) - max(3.0, MARGIN * h(512)) - eps], 5, ("edge", 25.0, 1, 0.95), 500.0, None, few),
        "margin-32-over": ("base", [float(b[2048]) - max(30.0, MARGIN * h(2048)) - eps], 5, ("edge", 25.0, 2, 1.05), 500.0, None, few),
        "margin-32-cold": ("base", [float(b[2048]) - max(30.0, MARGIN * h(2048)) - eps], 5, 2, 500.0, None, few),
        # cut-off 200: two lines 2 x cut apart in one call, both cut-off edges inside the grid
        "cut-200-pair": ("base", [BASE_NU0 - 150.0, float(b[-1]) + 150.0], 5, 0, 200.0, None, every),
        "exactly-cut-hi-200": ("base", [float(b[-1]) + 200.0], 1, 4, 200.0, None, ["default"]),
        # k_linesum: cut-off 100, and tiles wider than 27 cm^-1
        "cut-100": ("base", [float(b[50 * 64 + 32])], 5, 0, 100.0, None, few),
        "wide-tiles": ("wide", [float(g["wide"][1200]) + 0.1], 1, 0, 500.0, None, ["default"]),
        # below the cut-off: the 4-term body in every uniform set
        "low-near-lo": ("low", [float(low[400]) + 0.011], 5, 0, 500.0, None, few),
        "low-near-hi": ("low", [float(low[-400]) - 0.011], 5, 3, 500.0, None, few),
        "high-mid": ("high", [float(g["high"][50 * 64 + 32]) + 0.003], 5, 5, 500.0, None, few),
        "geo-mid": ("geo", [float(g["geo"][3000]) + 0.003], 5, "calm", 500.0, None, few),
        "geo-mid-cold": ("geo", [float(g["geo"][3000]) + 0.003], 5, 2, 500.0, None, few),
        "short-mid": ("short", [float(g["short"][40]) + 0.003], 1, 4, 500.0, None, few),
    }
    # own range minus parent's ("low": [lo, pa) below the parent's range, "high": [pb, hi) above it).  A range's low end is measured from the
    # interval's last point on the left (nu_hi - D_far) and on the right (nu_hi + D_near), its high end from the first point.  Just above
    # nu[4031] lies the end of a LOWER-half interval of every size from 64 to 2048 points (4032 / size is odd), just above nu[4096] the start
    # of every size's first interval whose UPPER-half sibling starts one size further: a line a bound away from there is in the child's
    # range and not in the parent's at every size at once
    far, near = (30.0, 120.0, 500.0), D_NEAR
    for r in (1, 2, 3):
        out[f"left-low-{r}"] = ("base", [float(b[4031]) + eps - far[r - 1]], 1, r, 500.0, None, every)
        out[f"right-low-{r}"] = ("base", [float(b[4031]) + eps + near[r - 1]], 1, r + 1, 500.0, None, every)
        out[f"left-high-{r}"] = ("base", [float(b[4096]) + eps - near[r - 1]], 1, r + 2, 500.0, None, every)
        out[f"right-high-{r}"] = ("base", [float(b[4096]) + eps + far[r - 1]], 1, r + 3, 500.0, None, every)
    # clusters: 60 cm^-1 below the grid the real line is in region 2 (32 nodes) of the first intervals and region 3 (32, 16) of the others
    for at in CLUSTER_AT:
        out[f"cluster-{at}"] = ("base", [BASE_NU0 - 60.0], 1, 4, 500.0, at, ["default", "interp-off"] if at else every)
    return out


COLUMN_K = 17
COLUMN_SEED = {"col/first": "calm", "col/second": 2, "col/cut-100": 2, "col/graph": 2}      # (col/first: no wide state, every region interpolated)


class Cases:
    """the cases by name, built on first use and kept: the placements (cs_shape_batch, cs_shape_points) and "col/first", "col/second" (a
    17-level column with the PHCO2 gas first, or second behind a Voigt gas whose one line reaches no point of the grid), "col/cut-100" and
    "col/graph" (the column a captured step is replayed on after its states turn cold and thick)"""

    def __init__(self, cs):
        self.cs, self._made, self.grids = cs, {}, grids()
        self.place = placements(self.grids)

    def names(self):
        return list(self.place) + ["col/first", "col/second", "col/cut-100", "col/graph"]

    def runs(self, name):
        return [RUN[r] for r in (self.place[name][6] if name in self.place else ["default", "interp-off", "own-core", "tiles-as-intervals"])]

    def __getitem__(self, name):
        if name not in self._made:
            self._made[name] = self._make(name)
        return self._made[name]

    def _make(self, name):
        cs = self.cs
        if name in self.place:
            gname, cen, K, seed, cut, at, _ = self.place[name]
            return Case(cs, name, self.grids[gname], [line_table(cs, cen, at)], states(K, seed), cut=cut, ksel=compared(K),
                        points_only=name.startswith("exactly-cut"))
        _, _, sts = column_states(cs, COLUMN_K, COLUMN_SEED[name])
        b = self.grids["base"]
        # (col/graph: the line of margin-32-cold, whose 25 K, 3e6 Pa state is the column's last level)
        ph = line_table(cs, self.place["margin-32-cold"][1] if name == "col/graph" else [float(b[50 * 64 + 32]) + 0.007])
        cut = 100.0 if name == "col/cut-100" else 500.0
        tabs = [I.one_line_table(cs, BASE_NU0 - 100.0, iso=2), ph] if name == "col/second" else [ph]
        return Case(cs, name, b, tabs, sts, cut=cut, concs=[CONC] * len(tabs), ksel=compared(COLUMN_K))
