"""The per-(state, line) parameter stage on the device -- prep_body of csrc/cs_kernels.h with the host tables of cs_api.hip behind it --
one line at a time against the 40-digit values of tests/lineparam_ref.py, within its derived bound (lineparam_bound, c0 = C0_GPU):
every isotopologue of data/molparam.json with a fit, the edge values of every line parameter under codes 0, 1, 2, 4, 5, 6 and under
CS_SHAPE_PSHIFT and code 7 on a table read from a .par file, state sets on both sides of a chunk of
CS_PREP_KC = 8 states, and columns that fill all CS_MAX_GAS = 16 gas slots, merged and unmerged, code 7 among the members.  Tables are synthetic, with lines
spaced so that every probe sees exactly one line of a table (tests/test_lineparam_ref.py counts them); grids hold only the probes, so
every call takes the short-grid forms.  Each test prints its worst error / bound."""
import ctypes as C

import numpy as np
import pytest

import lineparam_ref as R
from test_gpu_pressure_shift import write_par

pytestmark = pytest.mark.gpu

NAMES = {0: "voigt", 1: "lorentz", 2: "doppler", 4: "voigtCKD", 5: "voigtVVH", 6: "voigtCKDVVH", 7: "voigtLBL"}
EINVAL, ENOCHEB = -1, -3


@pytest.fixture(scope="module")
def ctx(cs):
    c = cs.Context(0)
    yield c
    c.close()


def run_calls(cs, ctx, code, sl, sts, cut):
    """the probes of one table and state set through cs_shape_batch and cs_shape_points: (got_batch, got_points, want, bound, zero)"""
    lines = [R.line_of(sl, l) for l in range(len(sl.nu))]
    psh = bool(code & R.PSHIFT)
    code &= ~R.PSHIFT
    # (pedestal codes: also 0.9 cut, and beyond the cut-off an exact 0; shifted codes: probes about the state's own shifted centre)
    nu, pr = R.probes(lines, sts, code, cut, far=code in (4, 6, R.LBL), centres=R.shifted_centres(sl, sts) if psh or code == R.LBL else None)
    want, bnd, zero = R.expected(code | (R.PSHIFT if psh else 0), sl, sts, nu, pr, cut)
    T, P, Pp = (np.array(x) for x in zip(*sts))
    k, i = np.array([p[0] for p in pr]), np.array([p[1] for p in pr])
    a = cs.shape_batch(sl, NAMES[code], nu, T, P, Pp, cut, ctx, pressure_shift=psh)
    b = cs.shape_points(sl, NAMES[code], nu, T, P, Pp, cut, ctx, pressure_shift=psh)
    return a[k, i], b[k, i], want, bnd, zero


def test_every_isotopologue(cs, ctx):
    """one line per isotopologue with a fit, every molecule, Lorentz, Doppler and Voigt at the ends of the fit's range, Tref and two
    seeded temperatures: its own molar mass (alpha), its own row of the [niso][16] fit table (S)"""
    acc = {c: [[], [], [], []] for c in (0, 1, 2)}
    worst = {}
    n = 0
    for M in sorted(cs.MOLPARAM):
        if not np.any(cs.MOLPARAM[M].hascheb):
            continue
        sl = R.iso_table(cs, M)
        n += len(sl.nu)
        for code in acc:
            a, b, want, bnd, zero = run_calls(cs, ctx, code, sl, R.iso_states(), R.CUT_ISO)
            for got in (a, b):
                for lst, x in zip(acc[code], (got, want, bnd, zero)):
                    lst.append(x)
    for code in acc:
        worst[code] = R.check(*[np.concatenate(x) for x in acc[code]], what=NAMES[code])
    print(f"{n} isotopologues; worst error / bound: " + ", ".join(f"{NAMES[c]} {w:.3f}" for c, w in worst.items()))
    assert n == sum(int(np.sum(m.hascheb)) for m in cs.MOLPARAM.values())


def test_isotopologue_without_fit_is_refused(cs, ctx):
    """an isotopologue without a Qref/Q fit still raises CS_ENOCHEB"""
    hit = 0
    for M, mpar in cs.MOLPARAM.items():
        for i in np.nonzero(~mpar.hascheb)[0]:
            sl = R.table(cs, M, [i + 1], [1000.0], 1e-21, 0.07, 0.09, 100.0, 0.7)
            with pytest.raises(cs.ClearSkyHIPError) as e:
                cs.shape_batch(sl, "voigt", np.array([999.9, 1000.0]), [296.0], [1e5], [10.0], 2.0, ctx)
            assert e.value.code == ENOCHEB
            hit += 1
    assert hit > 0


@pytest.mark.parametrize("code", [0, 1, 2, 4, 5, 6], ids=lambda c: NAMES[c])
def test_edge_parameters(cs, ctx, code):
    """nul from 0.05 to 15000 cm^-1, Epp = -1, 0, 1e-3 ... 2e4, na <= 0, gamma_self = 0, S = 1e-30 and 1e-19, T at both ends of the fit,
    P from 1e-2 to 1e7 Pa (and vacuum for Doppler and Voigt), K = 1, 7, 8, 9, 17 states.  Lorentz and Doppler are held to about
    (20 + terms) x 2^-53; the Voigt codes to that plus the 2e-13 Faddeeva allowance, which dominates.  The bound of codes 5 and 6 has NO
    cancellation term (1 + x) / (e^x - 1) at T (lineparam_bound): at nul = 0.05 cm^-1 and T = 1000 K that term alone is 1.4e4 x 2^-53 =
    1.5e-12, several times the allowance, so the (1 - exp(b/T)) form in the VVH branch would fail here at the low positions"""
    acc = [[], [], [], []]
    for sl, K, seed in R.edge_tables(cs):
        sts = R.states(K, seed, with_vacuum=code != 1)
        a, b, want, bnd, zero = run_calls(cs, ctx, code, sl, sts, R.CUT_EDGE)
        for got in (a, b):
            for lst, x in zip(acc, (got, want, bnd, zero)):
                lst.append(x)
    got, want, bnd, zero = (np.concatenate(x) for x in acc)
    worst = R.check(got, want, bnd, zero, what=NAMES[code])
    print(f"{NAMES[code]}: {len(want)} probes, underflow class {100 * R.split(want[~zero])[1]:.1f} %, worst error / bound {worst:.3f}")


@pytest.fixture(scope="module")
def shifted(cs, tmp_path_factory):
    return R.shifted_table(cs, tmp_path_factory.mktemp("lineparam"))


@pytest.mark.parametrize("code", [0, 1, 2], ids=lambda c: NAMES[c] + "-shifted")
def test_edge_parameters_pressure_shift(cs, ctx, shifted, code):
    """codes 0-2 with CS_SHAPE_PSHIFT on a table read from a small .par file: delta of both signs and 0, K = 8 and 17 states, probes about
    each state's own centre nul + delta P / P0 -- S, alpha and gamma stay those of the unshifted nul"""
    acc = [[], [], [], []]
    for K, seed in ((8, 1), (17, 2)):
        a, b, want, bnd, zero = run_calls(cs, ctx, code | R.PSHIFT, shifted, R.states(K, seed, with_vacuum=code != 1), R.CUT_EDGE)
        for got in (a, b):
            for lst, x in zip(acc, (got, want, bnd, zero)):
                lst.append(x)
    got, want, bnd, zero = (np.concatenate(x) for x in acc)
    worst = R.check(got, want, bnd, zero, what=NAMES[code])
    print(f"{NAMES[code]}, shifted: {len(want)} probes, worst error / bound {worst:.3f}")
    # the line whose shifted centre leaves the strict end-point filter in the 2 atm state only (lineparam_ref.FILTER_*): the vector method
    # gives an exact 0 in that state and the full value in the others; the scalar method, which has no pre-filter, the full value everywhere.
    # This is a check of codes 0 and 1 (see below for code 2)
    nu, sts = np.array(R.FILTER_GRID), list(R.FILTER_STATES)
    pr = [(k, i, 5) for k in range(len(sts)) for i in range(len(nu))]
    want, bnd, zero = R.expected(code | R.PSHIFT, shifted, sts, nu, pr, R.FILTER_CUT)
    T, P, Pp = (np.array(x) for x in zip(*sts))
    a = cs.shape_batch(shifted, NAMES[code], nu, T, P, Pp, R.FILTER_CUT, ctx, pressure_shift=True).ravel()
    b = cs.shape_points(shifted, NAMES[code], nu, T, P, Pp, R.FILTER_CUT, ctx, pressure_shift=True).ravel()
    assert not zero[2] and np.all(zero[:2]) and np.sum(~zero) >= 4          # (state 0: only nu_N, at |nu - c| = cut exactly, is in reach)
    assert np.all(a[:3] == 0.0)
    if code == 2:   # only codes 0 and 1 exercise the filter.  The Doppler profile is an exact 0 in fp64 long before the cut-off, so the row
        return      # above is 0 with or without the filter: for code 2 it shows that the call runs and says nothing about the filter
    assert b[2] > 0.0
    R.check(b, want, bnd, zero, what="end-point case, scalar method")
    R.check(a[3:], want[3:], bnd[3:], zero[3:], what="end-point case, vector method")


def test_edge_parameters_voigt_lbl(cs, ctx, shifted):
    """code 7 on the same table: K = 8 and 17 states (vacuum among them), probes about each state's own centre -- the line at 0.05 cm^-1
    has its mirror term inside the cut-off at every probe -- also at 0.9 cut and beyond the cut-off, under lineparam_bound with its
    centre term for the direct and the mirror profile.  Then the end-point case: the pedestal takes the whole profile off exactly on
    the cut-off, so there the 40-digit value is 0 for both methods and the scalar method is held to the bound's absolute form"""
    acc = [[], [], [], []]
    for K, seed in ((8, 1), (17, 2)):
        a, b, want, bnd, zero = run_calls(cs, ctx, R.LBL, shifted, R.states(K, seed, with_vacuum=True), R.CUT_EDGE)
        for got in (a, b):
            for lst, x in zip(acc, (got, want, bnd, zero)):
                lst.append(x)
    got, want, bnd, zero = (np.concatenate(x) for x in acc)
    worst = R.check(got, want, bnd, zero, what="voigtLBL")
    print(f"voigtLBL: {len(want)} probes, underflow class {100 * R.split(want[~zero])[1]:.1f} %, worst error / bound {worst:.3f}")
    nu, sts = np.array(R.FILTER_GRID), list(R.FILTER_STATES)
    pr = [(k, i, 5) for k in range(len(sts)) for i in range(len(nu))]
    infos = []
    want, bnd, zero = R.expected(R.LBL, shifted, sts, nu, pr, R.FILTER_CUT, infos=infos)
    T, P, Pp = (np.array(x) for x in zip(*sts))
    a = cs.shape_batch(shifted, "voigtLBL", nu, T, P, Pp, R.FILTER_CUT, ctx).ravel()
    b = cs.shape_points(shifted, "voigtLBL", nu, T, P, Pp, R.FILTER_CUT, ctx).ravel()
    assert np.all(zero[:3]) and np.sum(~zero) >= 3 and infos[2]["rel"] == 0.0 and infos[2]["mag"] > 0.0
    assert np.all(a[:3] == 0.0) and np.all(b[:2] == 0.0)
    edge = (R.U * (R.C0_GPU + R.model_terms(infos[2])) + R.FADDEEVA) * infos[2]["mag"]
    print(f"voigtLBL, end-point case: scalar method on the cut-off {b[2]:.3e}, allowed {edge:.3e}")
    assert 0.0 <= b[2] <= edge
    w = max(R.check(b[3:], want[3:], bnd[3:], zero[3:], what="end-point case, scalar method"),
            R.check(a[3:], want[3:], bnd[3:], zero[3:], what="end-point case, vector method"))
    print(f"voigtLBL, end-point case: worst error / bound {w:.3f}")


# ---- sixteen members ------------------------------------------------------------------------------------------------------------------

SHAPES = [(4, 3, 7), (5, 5, 17)]     # (np, nlobatto, K)


def _gases(cs, tabs, nu, shape, cut=R.CUT_MEMBERS, first=0):
    return [cs.DirectGas(sl, R.member_conc(first + m), nu, shape=shape, dnu_cut=cut) for m, sl in enumerate(tabs)]


def _column(cs, ctx, gases, npl, nlob, T0=230.0):
    P = cs.pressuregrid(50.0, 9e4, npl)
    T = T0 + 60.0 * (np.log(P / P[0]) / np.log(P[-1] / P[0]))
    return cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, nlob), ctx=ctx)


def _sigma(col):
    col.sigma_run()
    return col.sigma_nodes()


def _compare(col, tabs, codes, cuts, what, ref=None):
    want, bnd = ref or R.member_expected(tabs, codes, cuts, col.conc, col.Tk, col.Pk, col.nu)
    got = _sigma(col)
    r = np.abs(got - want) / np.abs(want) / (bnd + R.U * len(tabs))      # (+ one rounding per member added into the plane)
    assert np.all(want > R.UNDERFLOW)
    print(f"{what}: worst error / bound {np.max(r):.3f}")
    assert np.max(r) <= 1.0, what
    return got, (want, bnd)


@pytest.mark.parametrize("npl,nlob,K", SHAPES, ids=["K7", "K17"])
def test_sixteen_members(cs, npl, nlob, K):
    """all 16 gas slots, a different molecule and concentration function each: one merged Lorentz group of 16, one merged Voigt group, 16
    launch sets with merging off -- sum_g C_g sigma_g against the 40-digit sum; then other temperatures and concentrations through
    cs_column_update_state"""
    tabs = R.member_tables(cs)
    nu = R.member_grid(tabs)
    ctx = cs.Context(0)
    cuts = [R.CUT_MEMBERS] * 16
    for shape, code in (("lorentz", 1), ("voigt", 0)):
        col = _column(cs, ctx, _gases(cs, tabs, nu, shape), npl, nlob)
        assert col.K == K
        merged, ref = _compare(col, tabs, [code] * 16, cuts, f"{shape}, merged")
        info = col.info()
        assert info["groups"] == 1 and info["max_members"] == 16, info
    col.update(col.Tlev[::-1] + 11.0)       # (far from the first profile: every node's T, Pp and scale change)
    _compare(col, tabs, [0] * 16, cuts, "voigt, merged, after update_state")
    ctx.set_merge(False)
    col = _column(cs, ctx, _gases(cs, tabs, nu, "voigt"), npl, nlob)
    apart, _ = _compare(col, tabs, [0] * 16, cuts, "voigt, 16 groups", ref)      # (the same states as the merged Voigt column)
    assert col.info()["groups"] == 16
    assert np.max(np.abs(apart - merged) / merged) <= 2.0 * np.max(ref[1] + R.U * 16)      # (both within the bound of the same value)
    ctx.close()


MIXED = {0: "voigt", 1: "lorentz", 4: "voigtCKD", 5: "voigtVVH"}


def test_sixteen_members_mixed(cs):
    """codes 0, 1, 4, 5 side by side, two cut-offs, one slot named twice.  The expected launch groups follow the rule of cs_column_setup,
    written out here: a gas joins the first group of the same shape code and cut-off that does not hold its slot yet, else opens one"""
    tabs = R.member_tables(cs)
    tabs[15] = tabs[3]                                    # slot 3 named twice, with the shape and cut-off of its first use
    nu = R.member_grid(tabs)
    codes = [(0, 1, 4, 5)[m % 4] for m in range(16)]
    cuts = [2.0 if m < 8 else 3.0 for m in range(16)]
    cuts[15] = cuts[3]
    groups = []
    for m in range(16):
        for grp in groups:
            if grp["key"] == (codes[m], cuts[m]) and id(tabs[m]) not in grp["slots"]:
                grp["slots"].add(id(tabs[m]))
                break
        else:
            groups.append(dict(key=(codes[m], cuts[m]), slots={id(tabs[m])}))
    assert len(groups) == 9                               # 4 codes x 2 cut-offs, and the duplicate apart
    ctx = cs.Context(0)
    gases = [cs.DirectGas(tabs[m], R.member_conc(m), nu, shape=MIXED[codes[m]], dnu_cut=cuts[m]) for m in range(16)]
    col = _column(cs, ctx, gases, 4, 3)
    _compare(col, tabs, codes, cuts, "mixed line-up")
    info = col.info()
    assert info["groups"] == len(groups) and info["max_members"] == max(len(g["slots"]) for g in groups), info
    ctx.close()


def test_sixteen_members_with_voigt_lbl(cs, tmp_path):
    """the mixed line-up with member 6 as code 7, its table read from a .par file with shifts of both signs: nine launch groups, the
    code-7 member in one of its own, at K = 7 and 17 node states (arbitrary pressures: the centre term carries the rounding of
    nu -+ c as well)"""
    tabs = R.member_tables(cs)
    t, da = tabs[6], np.array([0.01, -0.005, 0.25])
    tabs[6] = cs.SpectralLines(write_par(str(tmp_path / "member6.par"), t.M, t.nu, t.S, t.gamma_a, t.gamma_s, t.Epp, t.na, da, t.I))
    assert np.array_equal(tabs[6].delta_a, da) and np.array_equal(tabs[6].nu, t.nu) and np.array_equal(tabs[6].I, t.I) and tabs[6].M == t.M
    nu = R.member_grid(tabs)
    codes = [(0, 1, 4, 5)[m % 4] for m in range(16)]
    codes[6] = R.LBL
    cuts = [2.0 if m < 8 else 3.0 for m in range(16)]
    ctx = cs.Context(0)
    gases = [cs.DirectGas(tabs[m], R.member_conc(m), nu, shape=NAMES[codes[m]], dnu_cut=cuts[m]) for m in range(16)]
    for npl, nlob, K in SHAPES:
        col = _column(cs, ctx, gases, npl, nlob)
        assert col.K == K
        _compare(col, tabs, codes, cuts, f"line-up with code 7, K = {K}")
        info = col.info()
        assert info["groups"] == 9 and info["max_members"] == 2, info      # 4 codes x 2 cut-offs, and code 7 apart
    ctx.close()


def test_sixteen_members_batch(cs):
    """cs_column_batch with B = 3 on the merged 16-member Voigt column: F equals three fresh columns to
    test_batched_columns_match_sequential's bound (1e-13 of the largest flux)"""
    tabs = R.member_tables(cs)
    nu = R.member_grid(tabs)
    ctx = cs.Context(0)
    gases = _gases(cs, tabs, nu, "voigt")
    col = _column(cs, ctx, gases, 4, 3)
    Ts = [col.Tlev + 0.0, col.Tlev[::-1] + 11.0, col.Tlev * 1.1 - 20.0]
    Fu, Fd = col.run_batch(Ts)
    for b, T in enumerate(Ts):
        one = cs.Column(col.P, 9.8, T, 0.029, 0.0, 0.0, *gases, core=cs.Discretized(3, 3), ctx=ctx)
        one.run()
        fu, fd = one.fetch()
        assert np.max(np.abs(Fu[b] - fu)) < 1e-13 * fu.max() and np.max(np.abs(Fd[b] - fd)) < 1e-13 * fu.max(), b
    ctx.close()


def test_merged_cache_eviction_is_bitwise(cs):
    """nine different 2-member columns in turn on one context, then the first again: the merged-table cache (CS_MAX_GAS / 2 entries)
    evicts and rebuilds; every result equals its first run bit for bit"""
    tabs = R.member_tables(cs)
    nu = R.member_grid(tabs)
    ctx = cs.Context(0)
    pairs = [(2 * q, 2 * q + 1) for q in range(8)] + [(0, 2)]
    first = []
    for a, b in pairs:
        g = [cs.DirectGas(tabs[a], R.member_conc(a), nu, dnu_cut=R.CUT_MEMBERS), cs.DirectGas(tabs[b], R.member_conc(b), nu, dnu_cut=R.CUT_MEMBERS)]
        col = _column(cs, ctx, g, 4, 3)
        first.append((g, _sigma(col)))
        assert col.info()["groups"] == 1 and col.info()["max_members"] == 2
    for g, s in first[:2] + first[-1:]:
        assert np.array_equal(_sigma(_column(cs, ctx, g, 4, 3)), s)
    ctx.close()


def test_seventeen_gases_are_refused(cs):
    """ngas = 17 > CS_MAX_GAS is CS_EINVAL from cs_column_setup, cs_fluxes_discretized and cs_fluxes_discretized_members"""
    tabs = R.member_tables(cs)
    nu = R.member_grid(tabs)
    ctx = cs.Context(0)
    col = _column(cs, ctx, _gases(cs, tabs, nu, "voigt"), 4, 3)
    L = cs.lib()
    n = 17
    slots = (C.c_int * n)(*([int(s) for s in col.slots] + [0]))
    shapes = (C.c_int * n)(*([0] * n))
    cuts = np.full(n, R.CUT_MEMBERS)
    conc = np.full(n * col.K, 1e-3)
    d = cs.dptr
    Tn, mun = np.asfortranarray(col.Tn).ravel(order="F").copy(), np.asfortranarray(col.mun).ravel(order="F").copy()
    Fu, Fd = np.zeros(col.np), np.zeros(col.np)
    setup = lambda ngas: L.cs_column_setup(ctx.handle, col.nnu, d(col.nu), None, col.np, d(col.P), 9.8, 3, d(Tn), d(mun), d(col.Tlev), ngas,
                                           slots, shapes, d(cuts), d(conc), 0.0, None, None, None, 0.841, 3, 0, 0)
    refused = lambda rc: rc == EINVAL and b"ngas out of range" in L.cs_last_error()      # (the count, and no other argument)
    assert refused(setup(n))
    assert refused(L.cs_fluxes_discretized(ctx.handle, col.nnu, d(col.nu), col.np, d(col.P), 9.8, 3, d(Tn), d(mun), d(col.Tlev), n, slots,
                                           shapes, d(cuts), d(conc), 0.0, None, None, None, 0.841, 3, None, None, None, d(Fu), d(Fd)))
    assert refused(L.cs_fluxes_discretized_members(ctx.handle, col.nnu, d(col.nu), col.np, d(col.P), 9.8, 3, d(Tn), d(mun), d(col.Tlev), n,
                                                   slots, shapes, d(cuts), d(conc), 0, None, None, 0, None, None, None, None, -1, 0.0, None,
                                                   None, None, 0.841, 3, None, None, None, d(Fu), d(Fd)))
    assert setup(16) == 0, L.cs_last_error()      # the very same arguments with ngas = CS_MAX_GAS are accepted
    ctx.close()
