"""Isolated lines on long grids: tables, grids, placements, probe sets and the per-form error model shared by
tests/test_isolated_line_ref.py (host) and tests/test_gpu_isolated_line.py (device).  The 40-digit values are lineparam_ref's
(sigma_isolated); nothing here reads the oracle or the GPU.

Inputs.  CO2-like tables (lineparam_ref.table) whose lines lie more than 2 x cut apart: every grid point is within the cut-off of at most
one line (the host test counts them with lines_within), so the device's value at a probe IS one line's term in one evaluation form.  Three
grids, each the smallest beyond the rules of cs_api.hip that select forms (SHORT_N, FOUR_N from the tile and level counts, long_n() from
the rule formulas as test_gpu_dispatch.py builds its grids); PLACEMENTS puts the centre of a line at the tile, interval and cut-off edges
of the short grid.  On those grids a point is 35 and more Doppler widths from the next, so a (line, state) has a handful of probes in the
line core; "col/fine" is the short grid's point count at a step of 2.5e-4 cm^-1, a third of a Doppler width, where the probes about the
centre (+-12 steps, the sub-tile ends of three tiles, both sides of s = 100 and 1e3) are all core probes of the six narrower states.  "col/fine-rep8" is that grid as long as voigt_plan (cs_api.hip) asks before a wave of k_voigt_near<0>, <1> takes eight tiles
in turn (rep_rules, rep_n) and one point more, with two lines (rep_centres) and the probes of the line core alone (core_probe_indices).

Clusters.  A piece of the matrix-core tables shorter than 8 lines is left to the vector unit (sepzones_body, edgezones_body: "too
short to be worth a wave's trip"), a window end goes to the 16 tile nodes from 16 lines on and is cut into phases from 48
(k_voigt_edge_mx), so ONE line never reaches k_cheb_nodes_mx, the window ends and middle pieces of k_voigt_edge_mx or its tile nodes.
The "-cluster" cases reach them: every line is followed, within one grid step, by GHOSTS = 63 lines of GHOST_RATIO = 1e-120 times its
strength.  The tables count 64 lines; the sum at a probe is still one line's, to 1e-100 (the host test bounds the ghosts' part with the
profile's largest ratio inside the cut-off).  The cases without a cluster hold one line per probe in the strict sense.

Probes (probe_indices) are a sample, per (line, state): +-12 grid steps about the centre; the two grid points on either side of each
distance where s = x^2 + y^2 crosses 100, 1e3, 1e4 and where |d| crosses R8, R4, R3 (series_radii.json; the state's own widths and its
group-of-16's widest, which the piece tables use); first and last point of every 64-point tile and of every interval of every level
within the cut-off, of the 8-point sub-tiles in the centre's tile and its neighbours; the last point inside and the first outside the
cut-off, the grid's ends; 32 log-spaced distances per side.  One test holds at most MAX_PROBES of them, so a call of K states is compared
in at most eight (STATES_COMPARED), and the long grid deals those eight out among its lines.

The sharp bound (every probe of the Voigt codes; s = x^2 + y^2 in the probe's state).  lineparam_bound keeps its rounding terms U (c0 +
terms) and loses the 2e-13 Faddeeva allowance F, which is replaced by what the sources state for the form that can serve the probe:

    form      truncation                              reciprocals                       roundings (2 per series term)
    vector    1e-15 (eps, series_radii.json) where    rcp_fast(s)                       2 x 4 U    far bodies of k_voigt_far, k_cheb_nodes
              s >= 1e6 (2, 3 terms); 1e-15 + 60 / s^4
              below (4 terms)
    near6     2e-15 (six terms at kSerS,              rcp_fast(s)                       2 x 6 U    near-zone pass of k_voigt_far, series of k_voigt_sub
              cs_faddeeva.h)
    matrix    1e-15                                   rcp_nr1 2e-15 (1/d^2 of the       2 x 4 U    k_cheb_nodes_mx, k_voigt_edge_mx (3, 4 terms)
                                                      record; w = 1/dnu^2 takes two
                                                      Newton steps: a rounding)
    matrix8   1e-15                                   the same                          2 x 8 U    the cores on the matrix pipe (8 terms)
    scalar    as `vector` where s >= 1e4              none (IEEE division)              2 x 4 U    the oracle (cs_oracle.c), which the host test holds
                                                                                                   to the same model
    mid       faddeeva_ref.bound(x, y, form, "mid"): the probe's own truncation and     100 <= s < 1e4: fad_mid -- tier 0 of k_voigt_near /
              rounding of the continued fraction, form "device" (rcp_nr) or "scalar"    k_voigt_near_both below 1e3; k_linesum's fad_re (the
                                                                                                   CS_SHAPE_PSHIFT groups) up to 1e4; the oracle
    near      faddeeva_ref.bound(x, y, form, "near"): trapezoid sum (24 x rcp_fast on   s < 100: fad_near -- tier 1 of the near-line kernels,
              the device) and pole term, each with its share of the 40-digit value      k_linesum's fad_re; the oracle

Below s = 1e3 nothing but `mid` and `near` serves a probe (k_voigt_sub and the near-zone pass hand those pairs over at kSerS); from 1e3
to 1e4 `near6`, the matrix forms and `mid` can; within S_EDGE = 1e-9 of a threshold the forms of both sides count, since the device's own
s (its alpha and x carry a few U) may fall on either.  Between 1e3 and 1e4 this model took the constant MID = 1e-14 (+ 8 U)
for the continued fraction; the per-probe figure of faddeeva_ref replaces it wherever it is the smaller one.  Where it is the larger --
at small y, where nr bi - ni br cancels to 1/19 of its parts and a worst case of every rounding gives up to 3.9e-14 -- the constant
stays as a cap (MID_CAP): a bound these probes are held to already does not widen (the device measures 5.5e-15 in that branch, the oracle
6.8e-15).  Below 1e3 no constant was ever asserted and the per-probe figure stands alone.  tests/phco2_line_ref.py, whose sharp model is
its own, takes allowance_s, the model as it was.

Two figures are not what was first assumed of them, and the model says so with the sources:
  - The four-term body between s = 1e4 and 1e6 is NOT inside eps: the first term it drops is u^4 p4(t), u = 1 / s, t = y^2 u in [0, 1],
    p4 = 59.0625 - 787.5 t + 2835 t^2 - 3780 t^3 + 1680 t^4 (the coefficients cs_kernels.h lists beside FarK), |p4| <= 59.0625 on [0, 1]:
    5.9e-15 at s = 1e4, which is what zone_compute's own comment says of that zone ("4-term series good to 1e-14") and what the oracle,
    which runs the same four terms, shows just beyond s = 1e4 (5.7e-15).  60 / s^4 covers it with the terms after it.
  - rcp_fast is NOT good to 3e-15 everywhere, as cs_faddeeva.h said: its seed is (float) s -- off by up to 2^-24 -- through v_rcp_f32,
    which the ISA gives to one ulp, 2^-23 / m relative with m in [1, 2) the mantissa of 1/s; one Newton step squares the sum:
    rcp_fast(s) = (2^-24 + 2^-23 / m)^2, from 1.4e-14 (m -> 2) to 3.2e-14 (1/s just above a power of two).  With 3e-15 in the model the
    vector forms went beyond the sharp bound by up to 1.2 at exactly such probes (s = 4.8e5, 1.25e8, 1.0e9: 1/s 7-8 % above 2^-19, 2^-27,
    2^-30) and nowhere else.  The header's comment is corrected with this model; the kernel is not changed (the figure is a per-line
    worst case of one sign that dense sums never meet, and a second Newton step is paid by every far pair).

A probe's form is not asked of the device: which of them can serve it follows from the settings of the run (RunForm) -- matrix cores
off leaves `vector` and `near6`; cs_shape_points runs the same machinery as cs_shape_batch (gas_states of cs_api.hip; only the
end-point filter differs) -- and the allowance is the largest among those, since the near-zone pass
and a core take whole tiles (a probe at s >= 1e4 shares its tile with a line inside dA).  Lorentz (code 1) has no series: its body is
the exact profile with rcp_nr1 (2e-15), already inside c0 of the hard bound -- a "sharp" bound of the hard one plus 2e-15 would say nothing,
so code 1 is held to the hard bound alone (about 4e-15; recorded ratio 0.94).  Sharp bounds of the Voigt codes: 2.8e-14 to 4.7e-14, up to
9e-14 at a margin of 15 per cent, against the hard 2e-13; below s = 1e3: 5e-15 to 4.5e-14.

Code 7 ("col/low-lbl": the low line of "col/low-ckdvvh" with a shift, read from a .par file) takes code 6's sharp bound with the centre
term of lineparam_bound among its rounding terms: the rounding of c = nul + delta P / P0 and of nu -+ c, times the slope of the direct and
of the mirror profile, each weighted by its share of the sum.  Probes and crossings are placed about the state's own shifted centre.

Interpolated probes.  A line is summed on the 64 Chebyshev nodes of interval I at level l where it is inside the cut-off of both ends of
I and at least max(dA, margin h) away (izone_frame, cs_kernels.h; h the half-width, dA = 100 alpha / sqrt(ln 2), here with the line's own
alpha <= the kernel's amax, so the set taken here contains the kernel's), at the largest such level in use.  The interpolant sum_m f(x_m)
l_m(nu) carries each node value's rounding with |l_m|: at most U x Lambda x max_I f, Lambda = (2/pi) ln 64 + 1 the Lebesgue constant of
64 Chebyshev nodes; relative to f(nu) that is U Lambda max_I f / f(nu).  A line outside I is monotone over it beyond the Doppler core, so
max_I f is its 40-digit value at the end of I nearest the line -- itself a probe (interval ends).  With the level cascade every smaller
level down to the last is one more such contraction (the child's maximum is below the parent's): the term counts once per level passed
-- up to four times the single-contraction formula: a deliberate widening, taken only by the runs in which the cascade can be on (with
cs_set_tuning key 12 = 2 the term counts once).
It is formed from reference values alone.

Recorded figures (worst error / bound per form; GPU run of this suite): see tests/test_gpu_isolated_line.py.
"""
import json
import math
import os

import numpy as np

import faddeeva_ref as FR
import lineparam_ref as R

U = R.U
CUT = 25.0
SQLN2 = math.sqrt(math.log(2.0))
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "series_radii.json")) as _f:
    _SR = json.load(_f)
EPS = float(_SR["eps"])
RADII = {int(n): (float(v["kSep"]), float(v["alpha_factor"])) for n, v in _SR["radii"].items()}
S_CROSS = (100.0, 1e3, 1e4)
S_SHARP = 1e3                                                       # (tests/phco2_line_ref.py: its own sharp model starts here)
S_EDGE = 1e-9                                                       # within this of a threshold in s the device's own s (its alpha, its x: some U each) may fall on either side
LEBESGUE = 2.0 / math.pi * math.log(64.0) + 1.0
RCP_NR1, TRUNC6, MID = 2e-15, 2e-15, 1e-14                        # cs_faddeeva.h: rcp_nr1, kSerS, the header's overall figure
MAX_PROBES = 2500
NP_COL = 61                                                         # levels; nlob = 2: K = 61 node states
STATES_COMPARED = (0, 15, 16, 17, 31, 32, 47, 60)
K_SETS = (1, 16, 17, 33)
P_LO, P_HI = 1.0, 3e6
CONC = 0.01

ALLOW = {      # without rcp_fast(s), which `vector` and `near6` add per probe
    "vector": EPS + 2 * 4 * U,
    "near6": TRUNC6 + 2 * 6 * U,
    "matrix": EPS + RCP_NR1 + 2 * 4 * U,
    "matrix8": EPS + RCP_NR1 + 2 * 8 * U,
    "lorentz": RCP_NR1,
}


def rcp_fast(s):
    """the bound of rcp_fast's relative error at s (module docstring): (2^-24 + 2^-23 / m)^2, m the mantissa of 1 / s"""
    m = math.frexp(1.0 / s)[0] * 2.0
    return (2.0 ** -24 + 2.0 ** -23 / m) ** 2


def radius(n, alpha, gamma):
    """R_n = kSep sqrt(gamma^2 + alpha_factor alpha^2) (sep_radii of cs_kernels.h without its 1e-6 safety)"""
    k, a = RADII[n]
    return k * math.sqrt(gamma * gamma + a * alpha * alpha)


def trunc4(s):
    """what the four-term series in 1 / s drops, relative: 60 / s^4 between s = 1e4 and 1e6 (module docstring), inside eps beyond; no
    four-term body serves s < 1e4 (there the allowance takes MID instead)"""
    return 60.0 / s ** 4 if 1e4 <= s < 1e6 else 0.0


def s_of(d, alpha, gamma):
    return (d * SQLN2 / alpha) ** 2 + (gamma * SQLN2 / alpha) ** 2


class RunForm:
    """what a run's settings allow to serve a probe: matrix (the matrix-core pieces and sub-tile cores), interp (interpolated wings, with
    `margin` as a fraction of the half-width and `first` the first level in use), cascade (levels folded into the smallest), scalar
    (the oracle: no reciprocal terms, its divisions are IEEE)"""

    def __init__(self, matrix=True, interp=True, margin=0.3, first=0, cascade=True, scalar=False):
        self.matrix, self.interp, self.margin, self.first, self.cascade, self.scalar = matrix, interp, margin, first, cascade, scalar

    def allowance_s(self, s, lorentz=False):
        """from s alone, with the constant MID between 1e3 and 1e4: what tests/phco2_line_ref.py (its own sharp model, s >= 1e3) takes"""
        if lorentz:
            return 0.0 if self.scalar else ALLOW["lorentz"]
        t4 = trunc4(s)
        if self.scalar:
            return (EPS + t4 if s >= 1e4 else MID) + 2 * 4 * U
        forms = [ALLOW["near6"] + rcp_fast(s)] + ([ALLOW["matrix"], ALLOW["matrix8"]] if self.matrix else [])
        forms.append(ALLOW["vector"] + t4 + rcp_fast(s) if s >= 1e4 else MID + 2 * 4 * U)
        return max(forms)

    def allowance(self, x, y, lorentz=False):
        """the Faddeeva allowance of a probe at (x, y), s = x^2 + y^2: the forms that can serve it (module docstring); within S_EDGE of a
        threshold, those of either side"""
        if lorentz:
            return 0.0 if self.scalar else ALLOW["lorentz"]
        s = x * x + y * y
        at = lambda S: abs(s / S - 1.0) < S_EDGE
        fform = "scalar" if self.scalar else "device"
        out = []
        if s >= 1e4 or at(1e4):              # the far bodies (the oracle: the same four terms, IEEE division)
            sf = max(s, 1e4)
            out.append((EPS + trunc4(sf)) + 2 * 4 * U if self.scalar else ALLOW["vector"] + trunc4(sf) + rcp_fast(sf))
        if (s >= 1e3 or at(1e3)) and not self.scalar:
            out += [ALLOW["near6"] + rcp_fast(s)] + ([ALLOW["matrix"], ALLOW["matrix8"]] if self.matrix else [])
        if (s < 1e4 or at(1e4)) and (s >= 100.0 or at(100.0)):
            mid = FR.bound(x, y, fform, "mid")
            out.append(min(mid, MID + 2 * 4 * U) if s >= 1e3 and not at(1e3) else mid)     # (MID_CAP, module docstring)
        if s < 100.0 or at(100.0):
            fr = 2.0 * x - math.floor(2.0 * x)       # (within S_EDGE of the grid choice's boundary: either grid)
            out += [FR.bound(x, y, fform, b) for b in (("near-int", "near-half") if min(abs(fr - 0.25), abs(fr - 0.75)) < S_EDGE else ("near",))]
        return max(out)


# ---- tables and states ----------------------------------------------------------------------------------------------------------------

GHOSTS, GHOST_STEP, GHOST_RATIO = 63, 1e-5, 1e-120


def one_line_table(cs, centres, iso=1, S=1e-20, ghosts=0):
    """one line per centre; ghosts: each followed by that many lines GHOST_STEP apart of GHOST_RATIO times its strength (module
    docstring: a cluster the piece tables count as lines, whose sum is one line's to 1e-100)"""
    centres = np.atleast_1d(np.asarray(centres, float))
    nu = np.concatenate([c + GHOST_STEP * np.arange(ghosts + 1) for c in centres])
    Sv = np.tile([S] + [S * GHOST_RATIO] * ghosts, len(centres))
    return R.table(cs, 2, [iso] * len(nu), nu, Sv, 0.07, 0.09, 300.0, 0.7)


def batch_states(K):
    """K states, pressures log-spaced over 1 .. 3e6 Pa (K = 1: 1e4 Pa), four temperatures in turn, Pp = CONC x P"""
    P = [1e4] if K == 1 else list(np.exp(np.linspace(math.log(P_LO), math.log(P_HI), K)))
    return [((200.0, 250.0, 296.0, 320.0)[k % 4], float(p), CONC * float(p)) for k, p in enumerate(P)]


def column_profile(cs):
    """(P levels, T levels) of the 61-level column: 1 Pa .. 3e6 Pa, T linear in ln P from 190 K to 330 K"""
    P = cs.pressuregrid(P_LO, P_HI, NP_COL)
    return P, 190.0 + 140.0 * np.log(P / P[0]) / math.log(P[-1] / P[0])


def compared(K):
    return [k for k in STATES_COMPARED if k < K]


# ---- grids ------------------------------------------------------------------------------------------------------------------------------

SHORT_DNU, SHORT_TILES = 0.025, 40
SHORT_N = 64 * SHORT_TILES + 1                     # 40 tiles and a last tile of one point
SHORT_NU0, LOW_NU0, HIGH_NU0 = 640.0, 0.5, 10000.0
FOUR_DNU, FOUR_N = 0.008, 8 * 1024 + 1              # eight intervals of the largest of four sizes, and a last one of one point
LONG_NU0, LONG_GAP = 600.0, 55.0
FINE_NU0, FINE_DNU = 666.68, 2.5e-4                 # a third of a Doppler width per point: the line core (s < 1e3) fills the centre's tiles


def grid(nu0, dnu, n):
    return nu0 + dnu * np.arange(n)


def tiles(n):
    return -(-n // 64)


def n_itot(sizes, n):
    return sum(-(-n // s) for s in sizes)


def long_rules(n, sizes, K=NP_COL):
    """the three rules of cs_api.hip the long grid is built from: one wave per (tile, state group) in k_voigt_edge_mx (mx_big, 1024
    blocks), one per (interval, group) in k_cheb_nodes_mx (2048 blocks), far_split 1 (16384 (tile, state) waves)"""
    g = -(-K // 16)
    return tiles(n) * g >= 1024, n_itot(sizes, n) * g >= 2048, tiles(n) * K >= 16384


def long_n(plan):
    """the smallest n with every rule of long_rules met; plan(n) = the interval sizes of an n-point grid (cs.interp_plan)"""
    ok = lambda n: all(long_rules(n, plan(n)))
    lo, hi = 1000, 200000
    assert not ok(lo) and ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return hi


def rep_rules(n, nlines, K=NP_COL):
    """the rule of cs_api.hip (voigt_plan) by which a wave of k_voigt_near<0>, <1> takes eight tiles in turn: half a million (tile, state)
    waves, or a quarter of a million with fewer lines than two per tile"""
    return tiles(n) * K >= 524288 or (nlines < 2 * tiles(n) and tiles(n) * K >= 262144)


def rep_n(nlines):
    """the smallest n that meets rep_rules"""
    ok = lambda n: rep_rules(n, nlines)
    lo, hi = 1000, 1000000
    assert not ok(lo) and ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return hi


REP_LINES, REP_TILE = 2, 1000                       # "col/fine-rep8": two lines; the first two points into this tile, the first of a wave's eight


def rep_centres(nu):
    """two points into tile REP_TILE (the core, +-90 points in the narrow states, lies in the last tile of one wave and the first of the
    next), and the middle of the last complete tile (the core reaches the ragged tile, where a wave's eight tiles end at the grid's)"""
    return [float(nu[64 * REP_TILE + 2]), float(nu[64 * (tiles(len(nu)) - 2) + 32])]


def long_centres(n):
    span = FOUR_DNU * (n - 1)
    return LONG_NU0 + 0.5 * LONG_GAP + 0.00317 + LONG_GAP * np.arange(int((span - 0.5 * LONG_GAP) // LONG_GAP) + 1)


# placements of one line on the short grid: name -> (centre, K of the state set its batch calls use)
def placements():
    nu = grid(SHORT_NU0, SHORT_DNU, SHORT_N)
    return {
        "mid-tile": (float(nu[20 * 64 + 32]), 33),
        "between-tiles-1024": (float(0.5 * (nu[1023] + nu[1024])), 17),
        "three-points-in": (float(nu[3]), 16),
        "outside-0.4cut": (SHORT_NU0 - 0.4 * CUT, 1),
        "edge-in-first-tile": (SHORT_NU0 - CUT + 0.5 * SHORT_DNU, 17),
        "exactly-cut": (SHORT_NU0 - CUT, 1),
    }


LOW_CENTRE = 3.0                                    # on the grid from 0.5: nu - cut <= 0, the mirror term of codes 5 and 6 in reach
LOW_DELTA = -0.01                                   # "col/low-lbl": the centre moves from 3.0 to 2.7 cm^-1 over the column's 1 Pa .. 3e6 Pa


def low_shifted_table(cs, directory):
    """one_line_table(cs, LOW_CENTRE) with the shift LOW_DELTA, written as a HITRAN 160-column file and read back (the library takes the
    shifts from the file alone; lineparam_ref.shifted_table's layout)"""
    path = str(directory) + "/isolated_low_shift.par"
    with open(path, "w") as f:
        r = (f"{2:2d}{R.ISOCHAR[0]}{LOW_CENTRE:12.6f}{1e-20:10.3E}{1.0:10.3E}{R._fx(0.07, 5, 4)}{R._fx(0.09, 5, 3)}{300.0:10.4f}"
             f"{R._fx(0.7, 4, 2)}{R._fx(LOW_DELTA, 8, 5)}")
        assert len(r) == 67, r
        f.write(r + " " * 93 + "\n")
    sl, ref = cs.SpectralLines(path), one_line_table(cs, LOW_CENTRE)
    assert np.array_equal(sl.delta_a, [LOW_DELTA]) and all(np.array_equal(getattr(sl, n), getattr(ref, n))
                                                           for n in ("nu", "S", "gamma_a", "gamma_s", "Epp", "na", "mu", "I"))
    return sl


# ---- probes -----------------------------------------------------------------------------------------------------------------------------

def _near(nu, v):
    """the two grid points on either side of v (those inside the grid)"""
    j = int(np.searchsorted(nu, v))
    return [i for i in (j - 1, j) if 0 <= i < len(nu)]


def probe_indices(nu, c, sizes, cut, crossings):
    """grid indices of the probes of one (line, state): c the (shifted) centre, crossings the distances whose two sides are taken"""
    n, h = len(nu), float(nu[1] - nu[0])
    inside = np.nonzero(np.abs(nu - c) <= cut)[0]
    out = {0, n - 1}
    ic = int(round((c - nu[0]) / h))
    out.update(i for i in range(ic - 12, ic + 13) if 0 <= i < n)
    for d in crossings:
        for sg in (-1.0, 1.0):
            out.update(_near(nu, c + sg * d))
    if inside.size:
        a, b = int(inside[0]), int(inside[-1])
        out.update(i for i in (a - 1, a, b, b + 1) if 0 <= i < n)
        for size in (64,) + tuple(sizes):
            for t in range(a // size, b // size + 1):
                for i in (t * size, min(t * size + size - 1, n - 1)):
                    if a <= i <= b:
                        out.add(i)
        tc = min(max(ic, 0), n - 1) // 64
        for t in (tc - 1, tc, tc + 1):
            for q in range(8):
                for i in (64 * t + 8 * q, 64 * t + 8 * q + 7):
                    if 0 <= i < n:
                        out.add(i)
        for d in np.exp(np.linspace(math.log(h), math.log(cut), 32)):
            for sg in (-1.0, 1.0):
                i = int(round((c + sg * d - nu[0]) / h))
                if 0 <= i < n:
                    out.add(i)
    return sorted(out)


def subtile_ends(nu, c):
    """first and last point of the 8-point sub-tiles (the tiles' own ends among them) of the centre's tile and its two neighbours"""
    n = len(nu)
    tc = min(max(int(round((c - nu[0]) / float(nu[1] - nu[0]))), 0), n - 1) // 64
    return {i for t in (tc - 1, tc, tc + 1) for q in range(8) for i in (64 * t + 8 * q, 64 * t + 8 * q + 7) if 0 <= i < n}


def core_probe_indices(nu, c, cut, crossings, alpha, gamma):
    """the probes of probe_indices with s < 1e4 in the probe's state, the two sides of `crossings` (those up to s = 1e4: Case._build) and
    subtile_ends: what a case about the near-line kernels is for -- the tile and interval ends of the whole cut-off are col/long's"""
    keep = subtile_ends(nu, c) | {i for d in crossings for sg in (-1.0, 1.0) for i in _near(nu, c + sg * d)}
    return sorted(i for i in probe_indices(nu, c, (), cut, crossings) if i in keep or s_of(nu[i] - c, alpha, gamma) < 1e4)


def crossings_of(alpha, gamma, alpha_w, gamma_w, cut):
    """(distances, [(kind, threshold, distance)]): where s crosses S_CROSS and |d| crosses R8, R4, R3 of the state's own widths and of its
    group's widest -- those inside the cut-off (beyond it nothing is evaluated, and another line may be)"""
    out = []
    for S in S_CROSS:
        d2 = S * alpha * alpha / math.log(2.0) - gamma * gamma
        if d2 > 0.0:
            out.append(("s", S, math.sqrt(d2)))
    for n in (8, 4, 3):
        out.append(("R", n, radius(n, alpha, gamma)))
        out.append(("Rw", n, radius(n, alpha_w, gamma_w)))
    out = [c for c in out if c[2] <= cut]
    return [c[2] for c in out], out


class Case:
    """one (grid, lines, states, shape code): lines = [(line dict, concentration C_l, Pp / P of its gas)], states = [(T, P)]; `which` maps a
    line to the states it is compared in (default: every compared state).  C_l = None: a cs_shape_* call (no factor, Pp = frac x P).
    core_only: the probes of core_probe_indices instead of probe_indices."""

    def __init__(self, cs, nu, sizes, tables, states, code=0, cut=CUT, concs=None, fracs=None, ksel=None, which=None, core_only=False):
        self.nu, self.sizes, self.code, self.cut, self.tables = np.asarray(nu, float), tuple(sizes), code, cut, tables
        self.core_only = core_only
        self.states = [(float(T), float(P)) for T, P in states]
        self.K = len(self.states)
        self.lines, self.ghosts = [], []
        for g, sl in enumerate(tables):
            smax = float(np.max(sl.S))
            for j in range(len(sl.nu)):
                if sl.S[j] < 1e-60 * smax:
                    self.ghosts.append((float(sl.nu[j]), float(sl.S[j]) / smax))
                else:
                    self.lines.append((R.line_of(sl, j), None if concs is None else concs[g], CONC if fracs is None else fracs[g], g))
        self.ksel = compared(self.K) if ksel is None else list(ksel)
        self.which = which or (lambda l: self.ksel)
        self.psh = R.shifts(code)      # (CS_SHAPE_PSHIFT, or code 7)
        self._build()

    def centre(self, k, l):
        ln = self.lines[l][0]
        return ln["nu"] + (ln["delta"] * self.states[k][1] / R.KATM if self.psh else 0.0)

    def widths(self, k, l):
        ln, _, frac, _ = self.lines[l]
        T, P = self.states[k]
        return R.widths(ln, T, P, frac * P)

    def _build(self):
        pr, self.cross = [], {}
        for l in range(len(self.lines)):
            w = [self.widths(k, l) for k in range(self.K)]
            for k in self.which(l):
                grp = range(16 * (k // 16), min(16 * (k // 16) + 16, self.K))
                kw = max(grp, key=lambda q: radius(4, *w[q]))
                dist, named = crossings_of(*w[k], *w[kw], self.cut)
                if self.core_only:
                    named = [x for x in named if s_of(x[2], *w[k]) <= 1e4 * (1.0 + S_EDGE)]
                    dist = [x[2] for x in named]
                self.cross[(k, l)] = named
                c = self.centre(k, l)
                idx = core_probe_indices(self.nu, c, self.cut, dist, *w[k]) if self.core_only else probe_indices(self.nu, c, self.sizes, self.cut, dist)
                pr += [(k, i, l) for i in idx]
        reach = lambda k, i, l: abs(self.nu[i] - self.centre(k, l)) <= self.cut
        others = lambda k, i, l: any(reach(k, i, m) for m in range(len(self.lines)) if m != l)
        self.pr = sorted(p for p in set(pr) if reach(*p) or not others(*p))      # (a point beyond its line's cut-off that another line reaches is that line's)
        self.k = np.array([p[0] for p in self.pr])
        self.i = np.array([p[1] for p in self.pr])

    def reference(self):
        """40-digit values and the terms of the bounds at every probe (computed once, kept)"""
        if hasattr(self, "want"):
            return self
        n = len(self.pr)
        self.want, self.zero, self.s, self.infos = np.zeros(n), np.zeros(n, bool), np.zeros(n), []
        self.x, self.y = np.zeros(n), np.zeros(n)
        for q, (k, i, l) in enumerate(self.pr):
            ln, C, frac, _ = self.lines[l]
            T, P = self.states[k]
            self.want[q], v, info = R.sigma_isolated(self.code, self.nu[i], ln, T, P, frac * P, self.cut, 1.0 if C is None else C)
            self.zero[q] = v == 0
            self.infos.append(info)
            self.s[q] = s_of(self.nu[i] - self.centre(k, l), info["alpha"], info["gamma"])
            self.x[q], self.y[q] = abs(self.nu[i] - self.centre(k, l)) * SQLN2 / info["alpha"], info["gamma"] * SQLN2 / info["alpha"]
        # codes 4, 6 at |d| = cut exactly (the grids hold such points): profile - pedestal cancels to an exact 0, rel = 0, and no relative
        # bound exists -- the device's value there is rounding of the two terms; it must be finite and >= 0 (`void`), nothing more
        self.void = np.array([f["rel"] <= 0.0 for f in self.infos]) & ((np.abs(self.nu[self.i] - [self.centre(k, l) for k, _, l in self.pr]) <= self.cut)
                                                                         | ((self.code & ~R.PSHIFT) in (5, 6, 7)))
        for f in self.infos:
            f["rel"] = f["rel"] if f["rel"] > 0.0 else 1.0
        self.hard = np.array([R.lineparam_bound(f, R.C0_GPU) for f in self.infos])
        self._at = {p: q for q, p in enumerate(self.pr)}
        return self

    def conditioning(self, form):
        """per probe: U x Lebesgue x (the line's largest 40-digit value over the probe's interval at the level in use) / (its value at
        the probe) x (levels passed), 0 where no level of the run can interpolate the pair"""
        self.reference()
        out = np.zeros(len(self.pr))
        if not form.interp:
            return out
        n = len(self.nu)
        lev = list(self.sizes)[form.first:]
        for q, (k, i, l) in enumerate(self.pr):
            if self.zero[q] or self.want[q] < R.UNDERFLOW:
                continue
            c, al = self.centre(k, l), self.infos[q]["alpha"]
            dA = 0.0 if (self.code & ~R.PSHIFT) == 1 else 100.0 * al / SQLN2
            for j, size in enumerate(lev):
                a, b = (i // size) * size, min((i // size) * size + size - 1, n - 1)
                vlo, vhi = self.nu[a], self.nu[b]
                if abs(c - vlo) > self.cut or abs(c - vhi) > self.cut or vlo <= c <= vhi:
                    continue
                e = b if c > vhi else a
                if min(abs(c - vlo), abs(c - vhi)) < max(dA, form.margin * 0.5 * (vhi - vlo)):
                    continue
                qe = self._at.get((k, e, l))
                assert qe is not None, (k, e, l)          # (interval ends inside the cut-off are probes)
                out[q] = U * LEBESGUE * max(self.want[qe], self.want[q]) / self.want[q] * ((len(lev) - j) if form.cascade else 1)
                break
        return out

    def sharp(self, form, c0=R.C0_GPU):
        """(mask of the probes the sharp bound applies to, their bounds)"""
        self.reference()
        lor = (self.code & ~R.PSHIFT) == 1
        m = ~self.zero & (not lor)                              # (Lorentz: the hard bound is the sharp one, module docstring)
        cond = self.conditioning(form)
        b = np.array([(U * (c0 + R.model_terms(f)) + form.allowance(x, y, lor) + cd) / f["rel"]
                      for f, x, y, cd in zip(self.infos, self.x, self.y, cond)])
        return m, b

    def isolation(self):
        """the probes that do NOT see exactly one line (ghosts apart): lines of the case within the cut-off of the point, expected 1 inside
        the cut-off of its own line, else 0, from the state's own (shifted) centres; or another line's mirror term (nu + nul <= cut, codes
        5 and 6) in reach"""
        bad = []
        for k, i, l in self.pr:
            allc = [self.centre(k, m) for m in range(len(self.lines))]
            inside = abs(self.nu[i] - self.centre(k, l)) <= self.cut
            if R.lines_within(allc, self.nu[i], self.cut) != (1 if inside else 0):      # (over the lines of every gas of the case)
                bad.append((k, i, l))
            if any(allc[m] + self.nu[i] <= self.cut for m in range(len(self.lines)) if m != l):
                bad.append((k, i, l))
        return bad


def _held(case, got, bounds, mask, what):
    """lineparam_ref.check on the probes of `mask`; a failure names the worst probe (state, point, line, offset, s, error, bound)"""
    try:
        return R.check(got[mask], case.want[mask], bounds[mask], case.zero[mask], what=what)
    except AssertionError as e:
        m = mask & ~case.zero & (np.abs(case.want) >= R.UNDERFLOW)
        r = np.where(m, np.abs(got - case.want) / np.where(m, np.abs(case.want), 1.0) / bounds, 0.0)
        worst = [(int(case.k[q]), int(case.i[q]), case.pr[q][2], float(case.nu[case.i[q]] - case.centre(*case.pr[q][::2])), float(case.s[q]),
                  float(r[q] * bounds[q]), float(bounds[q])) for q in np.argsort(r)[::-1][:4] if r[q] > 1.0]
        raise AssertionError(f"{e}; beyond the bound at {int(np.sum(r > 1.0))} probes, worst (k, i, l, d, s, error, bound): {worst}") from None


def compare(case, got, form, what):
    """got[len(case.pr)] against the reference under both bounds; returns (worst error / hard bound, worst error / sharp bound) and
    raises AssertionError beyond either"""
    case.reference()
    got = np.asarray(got, float)
    assert np.all(np.isfinite(got[case.void]) & (got[case.void] >= 0.0)), what
    hard = _held(case, got, case.hard, ~case.void, what + ", hard")
    m, b = case.sharp(form)
    sharp = _held(case, got, b, m & ~case.void, what + ", sharp")
    return hard, sharp


def core_ratio(case, got, form):
    """worst error / sharp bound over the probes of the line core alone (s < 1e3: fad_mid and fad_near), for the record; 0 without any"""
    m, b = case.sharp(form)
    sel = m & ~case.void & (case.s < S_SHARP) & (np.abs(case.want) >= R.UNDERFLOW)
    got = np.asarray(got, float)
    return float(np.max(np.abs(got[sel] - case.want[sel]) / np.abs(case.want[sel]) / b[sel])) if sel.any() else 0.0


# ---- the cases of the two test modules ----------------------------------------------------------------------------------------------------

def column_states(cs):
    """(P levels, T levels, [(T, P)] of the 61 node states) as cs.Column forms them (lobattoevaluations, nodepressures; nlob = 2)"""
    P, T = column_profile(cs)
    Tn, _ = cs.lobattoevaluations(P, cs.formprofile(P, T), cs.formprofile(P, 0.029), 2)
    return P, T, list(zip(cs.nodevalues(Tn, 2), cs.nodepressures(P, 2)))


MERGE_CONCS = (CONC, 0.02)


class Cases:
    """the cases by name, built on first use and kept: "batch/<placement>", "batch/low-vvh", "batch/fine" (cs_shape_batch, cs_shape_points) and
    "col/..." (a 61-state column)"""

    def __init__(self, cs, shifted=None, low_shifted=None):
        self.cs, self.shifted, self.low_shifted, self._made = cs, shifted, low_shifted, {}
        self.short = grid(SHORT_NU0, SHORT_DNU, SHORT_N)
        self.low = grid(LOW_NU0, SHORT_DNU, SHORT_N)
        self.four = grid(LONG_NU0, FOUR_DNU, FOUR_N)
        self.n_long = long_n(self.plan_of_n)
        self.long = grid(LONG_NU0, FOUR_DNU, self.n_long)

    def plan_of_n(self, n):
        return self.cs.interp_plan(grid(LONG_NU0, FOUR_DNU, n), CUT)

    def plan(self, nu):
        return self.cs.interp_plan(nu, CUT)

    def names(self):
        return ([f"batch/{p}" for p in placements()] + ["batch/low-vvh", "batch/fine", "col/short", "col/short-lorentz", "col/short-ckd", "col/low-vvh",
                "col/low-ckdvvh", "col/low-lbl", "col/short-shifted", "col/short-merge", "col/four", "col/long", "col/high", "col/short-cluster",
                "col/four-cluster", "col/long-cluster", "col/fine", "col/fine-rep8"])

    def __getitem__(self, name):
        if name not in self._made:
            self._made[name] = self._make(name)
        return self._made[name]

    def _make(self, name):
        cs = self.cs
        kind, what = name.split("/")
        if kind == "batch":
            if what == "low-vvh":
                sts = batch_states(16)
                return Case(cs, self.low, self.plan(self.low), [one_line_table(cs, LOW_CENTRE)], [(T, P) for T, P, _ in sts], code=5)
            if what == "fine":
                nu = grid(FINE_NU0, FINE_DNU, SHORT_N)
                return Case(cs, nu, self.plan(nu), [one_line_table(cs, float(nu[20 * 64 + 32]))], [(T, P) for T, P, _ in batch_states(33)])
            c, K = placements()[what]
            sts = batch_states(K)
            return Case(cs, self.short, self.plan(self.short), [one_line_table(cs, c)], [(T, P) for T, P, _ in sts])
        _, _, sts = column_states(cs)
        mid = placements()["mid-tile"][0]
        one = lambda nu, tabs, code=0, **kw: Case(cs, nu, self.plan(nu), tabs, sts, code=code, concs=[CONC] * len(tabs), **kw)
        gh = GHOSTS if what.endswith("-cluster") else 0
        what = what.replace("-cluster", "")
        if what == "short":
            return one(self.short, [one_line_table(cs, mid, ghosts=gh)])
        if what == "high":               # at 10000 cm^-1 the Doppler width, and with it the 3-term zone of the widest states, reaches the cut-off edge
            nu = grid(HIGH_NU0, SHORT_DNU, SHORT_N)
            return one(nu, [one_line_table(cs, float(nu[20 * 64 + 32]))])
        if what == "fine":               # the short grid's point count at 1/100 of its step: x = 0.3 .. 0.4 per point, every probe about the centre in the core
            nu = grid(FINE_NU0, FINE_DNU, SHORT_N)
            return one(nu, [one_line_table(cs, float(nu[20 * 64 + 32]))])
        if what == "fine-rep8":          # the fine grid as long as a wave of k_voigt_near<0>, <1> needs to take eight tiles, and one point more
            nu = grid(FINE_NU0, FINE_DNU, rep_n(REP_LINES) + 1)
            return one(nu, [one_line_table(cs, rep_centres(nu))], core_only=True)
        if what == "short-lorentz":
            return one(self.short, [one_line_table(cs, mid)], 1)
        if what == "short-ckd":
            return one(self.short, [one_line_table(cs, mid)], 4)
        if what == "low-vvh":
            return one(self.low, [one_line_table(cs, LOW_CENTRE)], 5)
        if what == "low-ckdvvh":
            return one(self.low, [one_line_table(cs, LOW_CENTRE)], 6)
        if what == "low-lbl":           # code 7: col/low-ckdvvh's line with a shift, read from a .par file (low_shifted_table)
            return one(self.low, [self.low_shifted], R.LBL)
        if what == "short-shifted":      # lineparam_ref.shifted_table: its line at 667 cm^-1 (delta = 0.01) is the one in reach of this grid
            return Case(cs, self.short, self.plan(self.short), [self.shifted], sts, code=R.PSHIFT, concs=[CONC], which=lambda l: compared(len(sts)) if l == 3 else [])
        if what == "short-merge":        # a second gas, its one line outside the grid and more than 2 cut from the first's
            tabs = [one_line_table(cs, mid), one_line_table(cs, SHORT_NU0 - 0.96 * CUT, iso=2, S=3e-21)]
            return Case(cs, self.short, self.plan(self.short), tabs, sts, concs=list(MERGE_CONCS), fracs=list(MERGE_CONCS))
        if what == "four":
            return one(self.four, [one_line_table(cs, float(self.four[4096 + 37]), ghosts=gh)])
        if what == "long":               # several lines 55 cm^-1 apart; the eight compared states are dealt out among them (MAX_PROBES)
            cen = long_centres(self.n_long)
            sel = compared(len(sts))
            deal = {l: [k for q, k in enumerate(sel) if (q < 6 and q // 2 == l) or (q >= 6 and q - 3 == l)] for l in range(len(cen))}
            return one(self.long, [one_line_table(cs, cen, ghosts=gh)], which=lambda l: deal[l])
        raise KeyError(name)
