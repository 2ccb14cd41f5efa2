"""Crowded line sums against 40-digit values: tables, probes, bounds and the restated density check shared by tests/test_crowded_line_ref.py
(host) and tests/test_gpu_crowded_lines.py (device).  Nothing here reads the oracle or the GPU; the 40-digit values are lineparam_ref's
(sigma_isolated), the grids, placements, probe sets and per-form error model are isolated_line_ref's.

Groups.  A crowd is a few GROUPS of lines: (centre, multiplicity M, strength ratio) -- M copies of one_line_table's line at one centre,
each of `ratio` times its strength.  Ratio 1 is a real line, GHOST_RATIO (1e-120) a filler the tables count and the sums do not see (a
filler group may give its M centres as an array).  Duplicated centres are legal input.  The exact sum at a probe is

    want = sum over real groups g of  M_g x sigma_isolated(line at c_g)

one 40-digit evaluation per (group, state, probe), whatever M is: a line lost from a group of 4095 moves the sum by 2.4e-4, one lost
from 9 by 0.11, against bounds of 1e-14 .. 5e-13.  The evaluations are kept per (grid, centre, states, code, probe set) in _PARTS, so a
sweep over M evaluates each centre once.

Bounds at a probe.  Each group's term carries the bound one isolated line has there (isolated_line_ref: the hard bound
lineparam_bound(c0), and the sharp bound with RunForm.allowance and the conditioning of interpolated probes, which is linear in the lines
and so weights like the rest); the sum of N terms >= 0 adds the summation term of any order of summation,

    bound = sum_g (M_g w_g / want) bound_g  +  gamma_(N-1),      gamma_n = n U / (1 - n U)

N = the table lines within the cut-off of the probe (lineparam_ref.lines_within over every line of the table, fillers included; a line of
codes 5, 6 whose mirror term counts -- nu + nul <= cut -- is two).  No form is given more than gamma_(N-1).  From M = 256 on (N - 1) U
is of the size of the sharp allowance itself (2.8e-14 at 257 against 2.8e-14 .. 4.7e-14), so there only the hard-bound comparison says
something: CrowdCase.sharp_held is False, compare() still returns both ratios and the tests print them.

A probe where one group's term is void (codes 4, 6 at |d| = cut exactly: isolated_line_ref.Case.reference) is void for the sum: finite
and >= 0.  Where no real line reaches a probe the value must be an exact 0 in tables without fillers.

The density check.  near_density restates check_near_density (csrc/cs_api.hip): with amax the widest Doppler width any state can have
(upper end of the grid + cut, TMAX, the table's lightest isotopologue), dA = 100 amax / sqrt(ln 2) (1 + 1e-6), r0 = sqrt(1e3) amax /
sqrt(ln 2) x 1.01 and span the widest 64-point tile, nzone = the most lines within span + 2 dA + 2 ds anywhere in the table must stay
below 2^20 and npt = the most within 2 r0 + 2 ds below 2^12 (the fields of the range word (first - N0) << 12 | count).  The cases are
constructed from it: which multiplicity is the last accepted, where the fillers of the offset case go, how far apart the two groups of
the shifted case sit.

Near-line pair counts.  tier_pairs counts, from the reference's own widths, the (point, line, state) triples with s = x^2 + y^2 < 100
(tier 1) and 100 <= s < 1e3 (tier 0) over the whole grid and every state; triples within S_EDGE of a threshold may fall on either side,
so the result is an interval per tier.
"""
import math

import numpy as np

import isolated_line_ref as I
import lineparam_ref as R
from clearsky_jl_amd import constants as C_
from clearsky_jl_amd import hitran as H

U = R.U
GHOST_RATIO = I.GHOST_RATIO
REAL_MIN = 1e-60                          # a group of at least this ratio is real (isolated_line_ref.Case draws the same line)
SHARP_M = 256                             # from this multiplicity on only the hard bound is asserted (module docstring)
FIRST_BITS, COUNT_BITS = 20, 12           # kNearFirstBits, kNearCountBits (csrc/cs_kernels.h)
NEAR_Q = 256                              # CS_NEAR_Q: queue entries per wave
S_SER, S_MID = 1e3, 100.0                 # kSerS, kMidS (csrc/cs_faddeeva.h)

M_THRESHOLDS = (7, 8, 9, 10, 11, 15, 16, 17, 47, 48, 49, 64, 65)
M_QUEUE = (3, 4, 5, 255, 256, 257, 4095)
M_REFUSED = 1 << COUNT_BITS
SPLITS = ((5, 3), (11, 5))
THREE = (100, 300, 100)
THREE_STEPS = 60
CODES = (4, 5, 6)
M_CODES = (9, 17)
M_BATCH = (257, 4095)
STEPS12 = 12


def gamma_n(n):
    """gamma_n = n U / (1 - n U): the relative error of a sum of n + 1 terms of one sign, in any order"""
    x = max(int(n), 0) * U
    return x / (1.0 - x)


def _members(groups):
    """[(centres array, ratio)] per group, in table order (ascending first centre)"""
    out = []
    for c, M, r in groups:
        cen = np.full(int(M), float(c)) if np.ndim(c) == 0 else np.asarray(c, float)
        assert len(cen) == int(M)
        out.append((cen, float(r)))
    return sorted(out, key=lambda g: float(g[0][0]))


def crowd_table(cs, groups, iso=1):
    """the table of groups = [(centre, multiplicity, strength_ratio)]: one_line_table's line parameters at every centre, strength x ratio"""
    mem = _members(groups)
    cen = np.concatenate([c for c, _ in mem])
    rat = np.concatenate([np.full(len(c), r) for c, r in mem])
    assert np.all(np.diff(cen) >= 0.0)
    one = I.one_line_table(cs, cen, iso=iso)
    return R.table(cs, 2, one.I, one.nu, one.S * rat, one.gamma_a, one.gamma_s, one.Epp, one.na)


# ---- the density check, restated ------------------------------------------------------------------------------------------------------------

def max_in(v, width):
    """the most lines of the ascending positions v in any window of `width` (check_near_density's two-pointer count: a line b counts
    those a <= b with not (v[b] - v[a] > width))"""
    v = np.asarray(v, float)
    a = np.searchsorted(v, v - width, side="left")
    while True:                                  # (v - width rounds; settle on the comparison the library makes)
        down = (a > 0) & ~(v - v[np.maximum(a - 1, 0)] > width)
        up = v - v[a] > width
        if not down.any() and not up.any():
            break
        a = a - down + (up & ~down)
    return int(np.max(np.arange(len(v)) - a + 1)) if len(v) else 0


def near_density(sl, nu, cut, ds=0.0):
    """check_near_density(G, nu, nnu, cut, ds) of csrc/cs_api.hip on the table sl (ascending): dict(amax, dA, r0, span, nzone, npt, ok)"""
    nu = np.asarray(nu, float)
    n = len(nu)
    i0 = np.arange(0, n, 64)
    span = float(np.max(nu[np.minimum(i0 + 63, n - 1)] - nu[i0]))
    amax = ((float(nu[-1]) + cut) / C_.c) * math.sqrt(2.0 * C_.R * H.TMAX / float(np.min(sl.mu)))
    dA = 100.0 * amax / I.SQLN2 * (1.0 + 1e-6)
    r0 = math.sqrt(S_SER) * amax / I.SQLN2 * 1.01
    nzone, npt = max_in(sl.nu, span + 2.0 * dA + 2.0 * ds), max_in(sl.nu, 2.0 * r0 + 2.0 * ds)
    return dict(amax=amax, dA=dA, r0=r0, span=span, nzone=nzone, npt=npt, ok=nzone < (1 << FIRST_BITS) and npt < (1 << COUNT_BITS))


# ---- one real line of a crowd at the crowd's probes ------------------------------------------------------------------------------------------

class _Part(I.Case):
    """isolated_line_ref.Case of ONE line; probes=None: its own probe set (the seed of a crowd's), else the (state, point) pairs given"""

    def __init__(self, cs, nu, sizes, centre, states, code, cut, C, frac, core_only, ksel, probes=None):
        self._fixed = probes
        super().__init__(cs, nu, sizes, [I.one_line_table(cs, centre)], states, code=code, cut=cut, concs=None if C is None else [C], fracs=[frac],
                         ksel=ksel, core_only=core_only)

    def _build(self):
        if self._fixed is None:
            return super()._build()
        self.cross = {}
        self.pr = [(k, i, 0) for k, i in self._fixed]
        self.k = np.array([p[0] for p in self.pr])
        self.i = np.array([p[1] for p in self.pr])


_PARTS = {}


def _part(cs, gkey, nu, sizes, centre, skey, states, code, cut, C, frac, core_only, probes=None):
    key = (gkey, float(centre), skey, code, cut, C, frac, core_only, None if probes is None else hash(tuple(probes)))
    if key not in _PARTS:
        if len(_PARTS) > 64:
            _PARTS.clear()
        _PARTS[key] = _Part(cs, nu, sizes, centre, states, code, cut, C, frac, core_only, list(skey[1]), probes)
    return _PARTS[key]


class CrowdCase:
    """one (grid, gases, states, shape code): gases = [groups] -- one table each (crowd_table), concs / fracs per gas as in
    isolated_line_ref.Case (concs None: a cs_shape_* call).  Probes: the union over the real groups' centres and the compared states
    of probe_indices (core_only: core_probe_indices; own=False: none of them), plus `steps` grid steps either side of every real centre and the points `extra`,
    in every compared state.  Quacks like isolated_line_ref.Case where test_gpu_isolated_line.run_column reads it (tables, nu, cut, K,
    k, i)."""

    def __init__(self, cs, name, nu, sizes, gases, states, code=0, cut=I.CUT, concs=(I.CONC,), fracs=None, core_only=False, ksel=None, steps=0, extra=(), own=True, tables=None):
        self.cs, self.name, self.nu, self.sizes, self.code, self.cut, self.core_only = cs, name, np.asarray(nu, float), tuple(sizes), code, cut, core_only
        self.states = [(float(T), float(P)) for T, P in states]
        self.K = len(self.states)
        self.ksel = I.compared(self.K) if ksel is None else list(ksel)
        self.gases = [list(g) for g in gases]
        self.concs = None if concs is None else list(concs)
        self.fracs = [I.CONC] * len(gases) if fracs is None else list(fracs)
        self.tables = [crowd_table(cs, g) for g in self.gases] if tables is None else list(tables)      # (tables: those of `gases`, made before)
        self.real = [(float(c), int(M), q) for q, g in enumerate(self.gases) for c, M, r in g if r >= REAL_MIN]
        assert all(r == 1.0 or r < REAL_MIN for g in self.gases for _, _, r in g)
        self.ghosts = [(c, int(M), r) for g in self.gases for c, M, r in g if r < REAL_MIN]
        self.M_max = max(M for _, M, _ in self.real)
        self.sharp_held = self.M_max < SHARP_M
        self._gkey = (float(self.nu[0]), float(self.nu[1] - self.nu[0]), len(self.nu))
        self._skey = (tuple(self.states), tuple(self.ksel))
        n, h = len(self.nu), float(self.nu[1] - self.nu[0])
        pts = set()
        for c in sorted({c for c, _, _ in self.real}):
            if own:
                pts.update((k, i) for k, i, _ in self._part(c, 0, None).pr)
            ic = int(round((c - self.nu[0]) / h))
            pts.update((k, i) for k in self.ksel for i in range(ic - steps, ic + steps + 1) if steps and 0 <= i < n)
        pts.update((k, int(i)) for k in self.ksel for i in extra)
        self.pr = sorted(pts)
        self.k = np.array([p[0] for p in self.pr])
        self.i = np.array([p[1] for p in self.pr])
        self.parts = [(self._part(c, q, self.pr), M) for c, M, q in self.real]

    def _part(self, c, q, probes):
        return _part(self.cs, self._gkey, self.nu, self.sizes, c, self._skey, self.states, self.code, self.cut,
                     None if self.concs is None else self.concs[q], self.fracs[q], self.core_only, probes)

    def all_centres(self):
        return np.concatenate([sl.nu for sl in self.tables])

    def counts(self):
        """N per probe: the table lines (every gas, fillers included) within the cut-off of the point, a line of codes 5, 6 whose mirror
        term counts (nu + nul <= cut) twice"""
        cen = self.all_centres()
        at = {}
        for i in sorted(set(int(i) for i in self.i)):
            v = self.nu[i]
            at[i] = R.lines_within(cen, v, self.cut) + (int(np.sum(cen + v <= self.cut)) if self.code in (5, 6) else 0)
        return np.array([at[int(i)] for i in self.i])

    def reference(self):
        """want, zero, void, N and the groups' shares of the sum at every probe (computed once, kept)"""
        if hasattr(self, "want"):
            return self
        for p, _ in self.parts:
            p.reference()
        terms = np.array([M * p.want for p, M in self.parts])
        self.want = terms.sum(axis=0)
        self.share = terms / np.where(self.want > 0.0, self.want, 1.0)
        self.zero = np.all([p.zero for p, _ in self.parts], axis=0)
        self.void = np.any([p.void for p, _ in self.parts], axis=0)
        self.N = self.counts()
        self.gamma = np.array([gamma_n(n - 1) for n in self.N])
        self.s = np.min([p.s for p, _ in self.parts], axis=0)           # the smallest s of any real line at the probe (for the record)
        return self

    def hard(self, c0=R.C0_GPU):
        self.reference()
        per = [np.array([R.lineparam_bound(f, c0) for f in p.infos]) for p, _ in self.parts]     # (f["rel"] > 0 after Case.reference)
        return np.sum(self.share * np.array(per), axis=0) + self.gamma

    def sharp(self, form, c0=R.C0_GPU):
        """(mask of the probes the sharp bound applies to, their bounds): the groups' own sharp bounds by their shares, plus gamma_(N-1)"""
        self.reference()
        mb = [p.sharp(form, c0) for p, _ in self.parts]
        m = ~self.zero & np.all([x[0] | p.zero for x, (p, _) in zip(mb, self.parts)], axis=0) & ((self.code & ~R.PSHIFT) not in (1, 2))      # (Lorentz, Doppler: the hard bound alone)
        return m, np.sum(self.share * np.array([x[1] for x in mb]), axis=0) + self.gamma

    def ghost_share(self):
        """an upper bound of the fillers' part of any probe's sum relative to one real line's term: (number of fillers) x (largest ratio) x
        the profile's largest ratio inside the cut-off, f(0) / f(cut), over the compared states (as test_isolated_line_ref.py bounds its clusters)"""
        if not self.ghosts:
            return 0.0
        p = self.parts[0][0]
        worst = 0.0
        for k in self.ksel:
            al, ga = p.widths(k, 0)
            worst = max(worst, float(R.fvoigt(R._m(0.0), R._m(al), R._m(ga)) / R.fvoigt(R._m(self.cut), R._m(al), R._m(ga))))
        return sum(M for _, M, _ in self.ghosts) * max(r for _, _, r in self.ghosts) * worst

    def tier_pairs(self):
        """((lo, hi) of tier 0, (lo, hi) of tier 1): the (point, line, state) triples with 100 <= s < 1e3 and with s < 100 inside the
        cut-off, over the whole grid, every state and every line of the first gas's table (its groups' widths are one line's); triples
        within S_EDGE of a threshold fall on either side"""
        p = self.parts[0][0]
        groups = [(np.full(int(M), float(c)) if np.ndim(c) == 0 else np.asarray(c, float)) for c, M, _ in self.gases[0]]
        lo0 = hi0 = lo1 = hi1 = 0
        ln, frac = p.lines[0][0], self.fracs[0]
        for k, (T, P) in enumerate(self.states):
            for cen in groups:
                for c, m in zip(*np.unique(cen, return_counts=True)):
                    al, ga = R.widths(dict(ln, nu=float(c)), T, P, frac * P)          # (the Doppler width is the centre's own)
                    d = self.nu - c
                    s = (d * I.SQLN2 / al) ** 2 + (ga * I.SQLN2 / al) ** 2
                    s = s[np.abs(d) <= self.cut]
                    below = lambda S, e: int(np.sum(s < S * (1.0 + e)))
                    lo1 += m * below(S_MID, -I.S_EDGE)
                    hi1 += m * below(S_MID, I.S_EDGE)
                    lo0 += m * (below(S_SER, -I.S_EDGE) - below(S_MID, I.S_EDGE))
                    hi0 += m * (below(S_SER, I.S_EDGE) - below(S_MID, -I.S_EDGE))
        return (lo0, hi0), (lo1, hi1)


def _ratio(case, got, bounds, mask, what, held=True):
    """worst |got - want| / want / bound over the probes of `mask`; held: lineparam_ref.check on them (exact zeros, the underflow class,
    the bound), a failure naming the worst probes (state, point, offset from the nearest real centre, N, error, bound)"""
    got = np.asarray(got, float)
    m = mask & ~case.zero & (np.abs(case.want) >= R.UNDERFLOW)
    r = np.where(m, np.abs(got - case.want) / np.where(m, np.abs(case.want), 1.0) / np.where(m, bounds, 1.0), 0.0)
    if held:
        try:
            R.check(got[mask], case.want[mask], bounds[mask], case.zero[mask], what=what)
        except AssertionError as e:
            cen = np.array(sorted({c for c, _, _ in case.real}))
            worst = [(int(case.k[q]), int(case.i[q]), float(np.min(np.abs(case.nu[case.i[q]] - cen))), int(case.N[q]), float(r[q] * bounds[q]),
                      float(bounds[q])) for q in np.argsort(r)[::-1][:4] if r[q] > 1.0]
            raise AssertionError(f"{e}; beyond the bound at {int(np.sum(r > 1.0))} probes, worst (k, i, |d|, N, error, bound): {worst}") from None
    return float(np.max(r)) if r.size else 0.0


def compare(case, got, form, what, c0=R.C0_GPU):
    """got[len(case.pr)] against M x the 40-digit values: (worst error / hard bound, worst error / sharp bound).  The hard bound is held
    at every probe; the sharp one where case.sharp_held (below SHARP_M copies), and is returned for the record otherwise.  Where no real
    line reaches, the value is an exact 0 (tables without fillers) or, with fillers, below 1e-100 of a line's strength."""
    case.reference()
    got = np.asarray(got, float)
    assert got.shape == case.want.shape and np.all(np.isfinite(got[case.void]) & (got[case.void] >= 0.0)), what
    if case.ghosts:
        assert np.all((got[case.zero] >= 0.0) & (got[case.zero] < 1e-100 * float(np.max(case.want)))), what
        got = np.where(case.zero, 0.0, got)
    hard = _ratio(case, got, case.hard(c0), ~case.void, what + ", hard")
    m, b = case.sharp(form, c0)
    sharp = _ratio(case, got, b, m & ~case.void, what + ", sharp", held=case.sharp_held)
    return hard, sharp


# ---- the offset field -----------------------------------------------------------------------------------------------------------------------

OFFSET_DNU, OFFSET_N, OFFSET_REAL = 0.5, 192, 3         # three tiles of 31.5 cm^-1; the real copies at the top point of the middle one
OFFSET_LEVELS = 3


def offset_grid():
    return I.grid(I.SHORT_NU0, OFFSET_DNU, OFFSET_N)


def offset_groups(cs, nu, more=0):
    """fillers spread evenly through one window of width span + 2 dA that starts dA below the middle tile -- its near zone for the widest
    Doppler width near_density takes -- with OFFSET_REAL real copies at the tile's top point, 2^20 - 1 + more lines in all.  The
    spacing follows from near_density's own span and dA; that npt stays below 2^12 is the host test's to assert."""
    d = near_density(I.one_line_table(cs, float(nu[127])), nu, I.CUT)
    width = d["span"] + 2.0 * d["dA"]
    top, lo = float(nu[127]), float(nu[64]) - d["dA"]
    n = (1 << FIRST_BITS) - 1 - OFFSET_REAL + more
    g = lo + width * (np.arange(n) + 0.5) / n                    # (half a spacing inside the window at both ends)
    below, above = g[g < top], g[g >= top]
    assert len(below) >= 1 << (FIRST_BITS - 1) and len(above) > 0 and above[0] > top
    return [(below, len(below), GHOST_RATIO), (top, OFFSET_REAL, 1.0), (above, len(above), GHOST_RATIO)]


def small_column_states(cs, nlev=OFFSET_LEVELS):
    """(P levels, T levels, [(T, P)] of the node states) of a column of nlev levels over isolated_line_ref's pressure range (nlob = 2)"""
    P = cs.pressuregrid(I.P_LO, I.P_HI, nlev)
    T = 190.0 + 140.0 * np.log(P / P[0]) / math.log(P[-1] / P[0])
    Tn, _ = cs.lobattoevaluations(P, cs.formprofile(P, T), cs.formprofile(P, 0.029), 2)
    return P, T, list(zip(cs.nodevalues(Tn, 2), cs.nodepressures(P, 2)))


# ---- the shifted pair ------------------------------------------------------------------------------------------------------------------------

SHIFT_DELTA = 0.001                                      # cm^-1 / atm: ds = delta x P_HI / atm = 0.0296 cm^-1 at the column's largest pressure


def shifted_pair(cs, directory, nu, centre, cut=I.CUT):
    """(table, distance, ds): two groups of M_REFUSED / 2 copies with the shift SHIFT_DELTA, written as a HITRAN 160-column file and read
    back (lineparam_ref.shifted_table's route: the library takes the shifts from the file alone).  Their distance is 2 r0 + ds rounded to
    the file's six decimals: between 2 r0 and 2 r0 + 2 ds, so that near_density counts M_REFUSED / 2 lines per 2 r0 without the shift
    and M_REFUSED with it."""
    ds = SHIFT_DELTA * I.P_HI / R.KATM
    r0 = near_density(I.one_line_table(cs, centre), nu, cut)["r0"]
    a = round(centre - 0.5 * (2.0 * r0 + ds), 6)
    b = round(a + 2.0 * r0 + ds, 6)
    path = str(directory) + "/crowded_shift.par"
    with open(path, "w") as f:
        for v in (a, b):
            r = (f"{2:2d}{R.ISOCHAR[0]}{v:12.6f}{1e-20:10.3E}{1.0:10.3E}{R._fx(0.07, 5, 4)}{R._fx(0.09, 5, 3)}{300.0:10.4f}"
                 f"{R._fx(0.7, 4, 2)}{R._fx(SHIFT_DELTA, 8, 5)}")
            assert len(r) == 67, r
            f.write((r + " " * 93 + "\n") * (M_REFUSED // 2))
    sl = cs.SpectralLines(path)
    assert len(sl.nu) == M_REFUSED and np.all(sl.delta_a == SHIFT_DELTA) and sorted(set(sl.nu)) == [a, b]
    return sl, b - a, ds


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------

class Cases:
    """the cases by name, built on first use and kept:
      thr/M<M>            short grid, M real copies at col/short-cluster's centre, a 61-state column        (piece thresholds)
      thr/split-<a>+<b>   a and b copies at centres one grid step apart
      thr/code<c>-M<M>    codes 4 (short grid), 5, 6 (col/low-vvh's grid and centre)
      q/M<M>              fine grid, one group mid-tile, core probes and +-12 steps                            (queue windows, count field)
      q/three             100, 300, 100 copies 60 grid steps apart
      q/rep8              the eight-tiles-per-wave grid, 257 copies at both rep_centres
      qb/M<M>-K<K>        cs_shape_batch / cs_shape_points states (batch_states(K)), fine grid
      pair/merge          two gases of M_REFUSED / 2 copies each at one centre
      off/batch, off/col  the offset field: 2^20 - 1 lines in the middle tile's near zone, three real copies at its top point
      full/code<c>        M_REFUSED copies (refused for the Voigt codes, accepted for 1 and 2), fine grid, core probes"""

    def __init__(self, cs):
        self.cs, self._made = cs, {}
        self.short = I.grid(I.SHORT_NU0, I.SHORT_DNU, I.SHORT_N)
        self.low = I.grid(I.LOW_NU0, I.SHORT_DNU, I.SHORT_N)
        self.fine = I.grid(I.FINE_NU0, I.FINE_DNU, I.SHORT_N)
        self.mid = I.placements()["mid-tile"][0]
        self.fine_mid = float(self.fine[20 * 64 + 32])
        self._sts = self._off = None

    def plan(self, nu):
        return self.cs.interp_plan(nu, I.CUT)

    def column(self):
        if self._sts is None:
            self._sts = I.column_states(self.cs)[2]
        return self._sts

    def names(self):
        return ([f"thr/M{M}" for M in M_THRESHOLDS] + [f"thr/split-{a}+{b}" for a, b in SPLITS] + [f"thr/code{c}-M{M}" for c in CODES for M in M_CODES]
                + [f"q/M{M}" for M in M_QUEUE] + ["q/three", "q/rep8"] + [f"qb/M{M}-K{K}" for M in M_BATCH for K in I.K_SETS])

    def __getitem__(self, name):
        if name not in self._made:
            self._made[name] = self._make(name)
        return self._made[name]

    def _make(self, name):
        cs = self.cs
        kind, what = name.split("/")
        col = lambda nu, groups, **kw: CrowdCase(cs, name, nu, self.plan(nu), [groups], self.column(), **kw)
        if kind == "thr":
            if what.startswith("M"):
                return col(self.short, [(self.mid, int(what[1:]), 1.0)])
            if what.startswith("split"):
                a, b = (int(x) for x in what[6:].split("+"))
                return col(self.short, [(self.mid, a, 1.0), (float(self.short[20 * 64 + 33]), b, 1.0)])
            code, M = int(what[4]), int(what.split("-M")[1])
            return col(self.short, [(self.mid, M, 1.0)], code=4) if code == 4 else col(self.low, [(I.LOW_CENTRE, M, 1.0)], code=code)
        if kind == "q":
            if what.startswith("M"):
                return col(self.fine, [(self.fine_mid, int(what[1:]), 1.0)], core_only=True, steps=STEPS12)
            if what == "three":
                c = 20 * 64 + 32
                return col(self.fine, [(float(self.fine[c + (j - 1) * THREE_STEPS]), M, 1.0) for j, M in enumerate(THREE)], core_only=True, steps=STEPS12)
            if what == "rep8":
                nu = I.grid(I.FINE_NU0, I.FINE_DNU, I.rep_n(I.REP_LINES) + 1)
                return col(nu, [(c, 257, 1.0) for c in I.rep_centres(nu)], core_only=True, steps=STEPS12)
        if kind == "qb":
            M, K = (int(x[1:]) for x in what.split("-"))
            sts = [(T, P) for T, P, _ in I.batch_states(K)]
            return CrowdCase(cs, name, self.fine, self.plan(self.fine), [[(self.fine_mid, M, 1.0)]], sts, concs=None, core_only=True, steps=STEPS12)
        if kind == "pair":       # two gases of half the refused count each at one centre (MERGE_CONCS, as col/short-merge)
            half = [(self.fine_mid, M_REFUSED // 2, 1.0)]
            return CrowdCase(cs, name, self.fine, self.plan(self.fine), [half, list(half)], self.column(), concs=I.MERGE_CONCS, fracs=I.MERGE_CONCS,
                             core_only=True, steps=STEPS12)
        if kind == "off":        # the offset field: offset_groups; K = 2 batch states or the five states of a 3-level column
            nu = offset_grid()
            if self._off is None:       # (a million lines: one table for both cases)
                groups = offset_groups(cs, nu)
                self._off = (groups, crowd_table(cs, groups))
            sts = [(T, P) for T, P, _ in I.batch_states(2)] if what == "batch" else small_column_states(cs)[2]
            return CrowdCase(cs, name, nu, self.plan(nu), [self._off[0]], sts, concs=None if what == "batch" else (I.CONC,), core_only=True,
                             ksel=range(len(sts)), steps=STEPS12, extra=(64, 127), tables=[self._off[1]])
        if kind == "full":       # (Doppler: the +-12 steps alone -- beyond them its values leave the doubles' range)
            code = int(what[4:])
            return col(self.fine, [(self.fine_mid, M_REFUSED, 1.0)], code=code, core_only=True, steps=STEPS12, own=code != 2)
        raise KeyError(name)
