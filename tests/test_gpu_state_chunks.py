"""States split into chunks: the three entry points that bound their per-state workspace (clearsky.jl_amd/csrc/cs_api.hip) -- the line
shapes (cs_shape_batch / cs_shape_points), the bake (cs_bake) and the batched column (cs_column_batch) -- run their states kc at a time,
with every per-state array, concentration and output row offset by the chunk's first state k0 and every workspace sized once for kc.

RULES writes out the three chunk rules (test_state_chunk_rules.py holds them to the source).  Each test computes kc for its own inputs and
asserts that they make at least three chunks with a ragged last one, with a margin of 10 % on the per-state bytes; the gridDim.y tests
reach the 65535 cap instead.  Large synthetic line tables (400 000 lines, some 19-29 MB of records per state) keep the state counts, and
so the reference work, small; the grids are short.  A chunk's workspace is the rule's budget, so the peak device memory of a test is
about 4 GiB (shapes, bake) to 9 GiB (column batch) by construction.

Every row (profile) is compared with the same states run in calls of fewer than kc states at 5e-13 of its largest value: the state count
of a launch feeds the per-launch form rules, so forms can differ between chunks and the comparison is not bitwise.  Rows on both sides
of each chunk boundary, the first and last and a few random ones are compared with the oracle at 1e-11 (Doppler 1e-9, as in
test_shape_batch_fuzz), codes 4-6 through tests/ckdvvh_ref.py on the magnitude scale of its `err`.

Shifted line centres (CS_SHAPE_PSHIFT on codes 0-2, and code 7) have a section of their own at the end: who is inside a cut-off
depends on the state there, so a chunk has state-dependent pieces of its own -- the records the strict pre-filter parks state by state,
the per-state fringe tests of the pedestal finish, and the largest shift ds of ALL K states, which widens every window, zone and interval
once.  Its table (354 128 lines at multiples of 2^-6, delta_a at multiples of 2^-5 with alternating signs, a pair of lines about every
limit of the pre-filter) is read from a .par file of 57 MB, written once per module (3 s); its states are dyadic multiples of P0 up to
2 atm, the first chunk at or below 0.5 atm, so a ds taken from one chunk is too small for another; grid, shifts and pressures are
exact in fp64 (voigt_lbl_ref.dyadic_premise, asserted on the rows compared) and the exact-shift bar of 1e-11 applies (Doppler 1e-9);
the bake's knots and the column's nodes are arbitrary pressures and take the 1e-9 of tests/test_gpu_voigt_lbl.py.  The sizes follow the
same rules (the shifts are per table, not per state; code 7 counts as ped): same peak memory.  test_state_chunk_rules.py checks without
a GPU that every such case crosses two boundaries, that membership by shifted centre differs from membership by table position among
the compared rows (direct and mirror), and that the pre-filter keeps a line in one compared row and drops it in another.

Recorded figures (MI355X).  Worst error: shapes 5.1e-15 (0 | 16, cut 25), 6.3e-15 (1 | 16, cut 5), 1.1e-15 (2 | 16, cut 25), 8.7e-15,
7.0e-15, 3.1e-14 (code 7, cut 5, 25, 0.25); ld_state padding 8.1e-15; bake 1.5e-11 (both codes: the knots' arbitrary pressures);
column batch, flux against the oracle column 9.2e-16 (0 | 16), 1.2e-15 (code 7), where the shifts move the flux by 1.0e-4 and 9.0e-5.
A seeded defect (a scratch build, not committed, that can only drop lines: gas_states taking ds from the pressures of its first chunk
alone): all six shifted shape cases, the padding case and both bakes fail -- the whole result differs from the small calls by 0.09 to
0.55 of a row's largest value -- while the 25 tests of this module that came before, tests/test_gpu_voigt_lbl.py,
tests/test_gpu_pressure_shift.py and tests/test_gpu_lineparams.py (53 tests) all pass: none of them runs a shifted call in more than
one chunk.  (With ds taken from the first STATE alone, those modules fail too: their states begin at the lowest pressure.)
"""
import os

import numpy as np
import pytest

import ckdvvh_ref as X
import test_gpu_pressure_shift as PS
import voigt_lbl_ref as V
import workloads as W
from conftest import HITRAN, relerr

pytestmark = pytest.mark.gpu

GIB = 1 << 30
HOT, COLD, F32, INT2, DBL = 32, 16, 16, 8, 8        # sizeof LineHot, LineCold, LineF32 (cs_kernels.h), int2, double
PED_B = 64                                          # CS_PED_B (cs_kernels.h)
GRID_Y = 65535


def ped_bytes(kn, L):
    """the pedestal workspace of kn states (cs_api.hip ped_bytes)"""
    return kn * (3 * L + (L + PED_B - 1) // PED_B) * DBL


# entry point -> (workspace budget, bytes per state).  L: the table's lines (column: the largest launch group's), ped: a code-4/6 group,
# mixed: cs_set_precision mode 1 (column only), vvh2: a second code-5/6 group (column only)
RULES = {
    "shape": (4 * GIB, lambda L, nnu, ped=False, **_: L * (HOT + COLD) + nnu * (DBL + INT2) + (ped_bytes(1, L) if ped else 0)),
    "bake": (4 * GIB, lambda L, nnu, ped=False, **_: L * (HOT + COLD) + nnu * INT2 + (ped_bytes(1, L) if ped else 0)),
    "column": (8 * GIB, lambda L, nnu, ped=False, mixed=False, vvh2=False:
               L * (HOT + COLD + (F32 if mixed else 0)) + nnu * INT2 + (ped_bytes(1, L) if ped else 0) + (nnu * DBL if vvh2 else 0)),
}


def chunk_size(rule, n, L, nnu, scale=1.0, **kw):
    """kc = min(n, budget / per_state, 65535) of the rule for n states; scale multiplies the per-state bytes"""
    budget, per_state = RULES[rule]
    return max(1, min(n, int(budget // int(per_state(L, nnu, **kw) * scale)), GRID_Y))


def boundaries(rule, n, L, nnu, **kw):
    """the chunk starts k0 > 0 of n states, after asserting three chunks or more, a ragged last chunk, and that both hold with 10 %
    fewer bytes per state"""
    kc = chunk_size(rule, n, L, nnu, **kw)
    b = list(range(kc, n, kc))
    assert len(b) >= 2, (rule, n, kc)
    assert (n - b[-1]) % 16 != 0, (rule, n, kc)
    assert n > 2 * chunk_size(rule, n, L, nnu, scale=0.9, **kw), (rule, n, kc)
    return kc, b


def states_for(rule, L, nnu, step=1, **kw):
    """the smallest multiple of step that makes three chunks even with 10 % fewer bytes per state, with a ragged last chunk"""
    hi = chunk_size(rule, 10 ** 7, L, nnu, scale=0.9, **kw)
    kc = chunk_size(rule, 10 ** 7, L, nnu, **kw)
    n = -(-(2 * hi + 1) // step) * step
    while (n % kc) % 16 == 0:
        n += step
    return n


NLINES = 400_000
GRID = 0.5 + 0.1 * np.arange(400)            # 0.5 .. 40.4 cm^-1: low lines reach the mirror terms of codes 5 and 6
GRID_CO2 = 600.5 + 0.1 * np.arange(400)
SHAPE_NAMES = {0: "voigt", 1: "lorentz", 2: "doppler", 3: "PHCO2", 4: "voigtCKD", 5: "voigtVVH", 6: "voigtCKDVVH", 7: "voigtLBL"}
FLAGS = {4: dict(ped=True, vvh=False), 5: dict(ped=False, vvh=True), 6: dict(ped=True, vvh=True), 7: dict(ped=True, vvh=True)}
PSHIFT = 16                                  # CS_SHAPE_PSHIFT (include/clearsky_hip.h)
KATM = V.KATM


@pytest.fixture(scope="module")
def big(cs):
    """400 000 synthetic lines over 0-25 000 cm^-1 (16 per cm^-1): H2O and CO2"""
    return {"H2O": cs.SpectralLines.synthetic(1, NLINES, 11, 0.0, 25000.0), "CO2": cs.SpectralLines.synthetic(2, NLINES, 12, 0.0, 25000.0)}


@pytest.fixture(scope="module")
def ctxs(cs):
    """interpolation on and off"""
    out = {}
    for on in (True, False):
        out[on] = cs.Context(0)
        out[on].set_interp(on)
    yield out
    for c in out.values():
        c.close()


class _Sub:
    pass


def _sub(sl, lo, hi):
    """the lines of sl in [lo, hi]: every line a grid with its cut-off reaches (the reference's work then follows the grid, not the table)"""
    a, b = np.searchsorted(sl.nu, [lo, hi])
    o = _Sub()
    for n in ("nu", "S", "gamma_a", "gamma_s", "Epp", "na", "mu", "I"):
        setattr(o, n, np.ascontiguousarray(getattr(sl, n)[a:b]))
    o.ncheb, o.cheb = sl.ncheb, sl.cheb
    o.delta_a = None if getattr(sl, "delta_a", None) is None else np.ascontiguousarray(sl.delta_a[a:b])
    return o


def _reach(sl, nu, cut):
    return _sub(sl, max(0.0, nu[0] - cut - 1.0), nu[-1] + cut + 1.0)


def _states(n, seed):
    """a different (T, P, Pp) in every row"""
    rng = np.random.default_rng(seed)
    T = rng.uniform(180.0, 330.0, n)
    P = 10.0 ** rng.uniform(1.0, 5.0, n)
    return T, P, P * 10.0 ** rng.uniform(-4.0, -1.3, n)


def _pieces(f, n, kc):
    """f(a, b) over [0, n) in calls of fewer than kc states (cut where the chunks are not), stacked"""
    m = max(1, kc // 2 + 3)
    assert m < kc
    return np.concatenate([f(a, min(n, a + m)) for a in range(0, n, m)])


def _close_rows(a, b, tol=5e-13):
    scale = np.max(np.abs(b), axis=1)
    assert np.all(np.isfinite(a)) and np.all(scale > 0)
    err = np.max(np.abs(a - b), axis=1) / scale
    assert np.max(err) < tol, (int(np.argmax(err)), float(np.max(err)))


def _check_rows(n, b0, seed):
    """both sides of every boundary, the first and last row, 8 random rows"""
    rng = np.random.default_rng(seed)
    r = {0, n - 1} | {k for k0 in b0 for k in (k0 - 1, k0)} | set(rng.choice(n, 8, replace=False).tolist())
    return sorted(r)


def _ref(cs, O, sl, code, nu, T, P, Pp, cut, strict):
    """(value, scale) of one state: the oracle for codes 0-3, ckdvvh_ref for codes 4-6"""
    if code in FLAGS:
        return X.expected(cs, O, sl, nu, T, P, Pp, cut=cut, strict=strict, **FLAGS[code])
    return O.shape_bang(SHAPE_NAMES[code], nu, sl, T, P, Pp, cut, strict_ends=strict), None


def _vs_ref(s, ref, code):
    val, scale = ref
    if code in FLAGS:
        return X.err(s, ref)
    assert np.array_equal(s == 0, val == 0)
    return relerr(s, val, floor=1e-280)


# (shape code, cut-off): H2O for every code but PHCO2 (CO2); 1, 5, 25 and 100 cm^-1 spread over the codes
SHAPE_CASES = [(0, 25.0), (0, 100.0), (1, 5.0), (2, 25.0), (3, 25.0), (4, 1.0), (4, 100.0), (5, 5.0), (5, 100.0), (6, 1.0), (6, 25.0)]


@pytest.mark.parametrize("code,cut", SHAPE_CASES, ids=[f"code{c}-cut{int(u)}" for c, u in SHAPE_CASES])
def test_shape_batch_and_points(cs, O, big, ctxs, code, cut):
    sl = big["CO2" if code == 3 else "H2O"]
    nu = GRID_CO2 if code == 3 else GRID
    ped = code in (4, 6)
    n = states_for("shape", NLINES, len(nu), ped=ped)
    kc, b0 = boundaries("shape", n, NLINES, len(nu), ped=ped)
    T, P, Pp = _states(n, 100 + code)
    sub = _reach(sl, nu, cut)
    rows = _check_rows(n, b0, code)
    tol = 1e-9 if code == 2 else 1e-11
    for fn, strict in ((cs.shape_batch, True), (cs.shape_points, False)):
        refs = {k: _ref(cs, O, sub, code, nu, T[k], P[k], Pp[k], cut, strict) for k in rows}
        for on, ctx in ctxs.items():
            s = fn(sl, code, nu, T, P, Pp, cut, ctx)
            assert s.shape == (n, len(nu))
            small = _pieces(lambda a, b: fn(sl, code, nu, T[a:b], P[a:b], Pp[a:b], cut, ctx), n, kc)
            _close_rows(s, small)
            for k in rows:
                e = _vs_ref(s[k], refs[k], code)
                assert e < tol, (fn.__name__, on, k, e)


def test_ld_state_padding(cs, O, big, ctxs):
    """ld_state > nnu across chunk boundaries (code 6: every offset of the shape path): the rows land at k ld_state, the padding columns
    keep their NaN"""
    sl, nu, cut, code = big["H2O"], GRID, 25.0, 6
    n = states_for("shape", NLINES, len(nu), ped=True)
    kc, b0 = boundaries("shape", n, NLINES, len(nu), ped=True)
    T, P, Pp = _states(n, 7)
    ctx = ctxs[True]
    ld = len(nu) + 37
    out = np.full((n, ld), np.nan)
    cs.check(cs.lib().cs_shape_batch(ctx.handle, ctx.slot_of(sl), code, cut, len(nu), cs.dptr(nu), n, cs.dptr(T), cs.dptr(P), cs.dptr(Pp),
                                     cs.dptr(out), ld))
    assert np.all(np.isnan(out[:, len(nu):]))
    _close_rows(out[:, :len(nu)], _pieces(lambda a, b: cs.shape_batch(sl, code, nu, T[a:b], P[a:b], Pp[a:b], cut, ctx), n, kc))
    sub = _reach(sl, nu, cut)
    for k in (b0[0] - 1, b0[0], b0[-1] - 1, b0[-1], n - 1):
        assert X.err(out[k, :len(nu)], X.expected(cs, O, sub, nu, T[k], P[k], Pp[k], cut=cut)) < 1e-11, k


@pytest.mark.parametrize("code", [0, 4, 6])
def test_bake(cs, O, big, code):
    """cs_bake over more knots than kc: ln sigma at every knot = ln of shape_batch at the knot state in calls of fewer than kc states (as
    test_bake does it); the oracle at the knots next to each boundary"""
    sl, nu, cut = big["H2O"], GRID, 25.0
    ped = code in (4, 6)
    nT = 17
    nP = -(-states_for("bake", NLINES, len(nu), step=nT, ped=ped) // nT)
    n = nT * nP
    kc, b0 = boundaries("bake", n, NLINES, len(nu), ped=ped)
    ctx = cs.Context(0)
    Om = cs.AtmosphericDomain((170.0, 330.0), nT, (10.0, 1e5), nP)
    g = cs.Gas(sl, 0.01, nu, Om, shape=SHAPE_NAMES[code], dnu_cut=cut, ctx=ctx, keep_host_tables=True)
    Z = g.lnsigma
    assert Z.shape == (len(nu), nT, nP) and not np.any(np.isnan(Z))
    TT, PP = np.meshgrid(Om.T, Om.P, indexing="ij")
    Tf, Pf = TT.ravel(order="F"), PP.ravel(order="F")
    s = _pieces(lambda a, b: cs.shape_batch(sl, code, nu, Tf[a:b], Pf[a:b], 0.01 * Pf[a:b], cut, ctx), n, kc)
    flat = s.T.reshape(len(nu), nT, nP, order="F")
    tiny = np.finfo(float).tiny
    z = (flat.reshape(len(nu), -1).min(axis=1) == 0) & (flat.reshape(len(nu), -1).max(axis=1) > 0)
    flat[z] = 0.0
    with np.errstate(divide="ignore"):
        ref = np.where(np.all(flat <= tiny, axis=(1, 2))[:, None, None], np.log(tiny), np.log(flat))
    assert np.array_equal(np.isfinite(Z), np.isfinite(ref))
    m = np.isfinite(ref) & (ref > np.log(tiny))
    assert np.max(np.abs(Z[m] - ref[m])) < 1e-12 * np.max(np.abs(ref[m]))
    sub = _reach(sl, nu, cut)
    for k in sorted({0, n - 1} | {k for k0 in b0 for k in (k0 - 1, k0)}):
        i, j = k % nT, k // nT
        r = _ref(cs, O, sub, code, nu, Om.T[i], Om.P[j], 0.01 * Om.P[j], cut, True)
        with np.errstate(divide="ignore"):
            e = _vs_ref(np.exp(Z[:, i, j]) * (Z[:, i, j] > np.log(tiny)), r, code)
        assert e < 1e-11, (k, e)
    ctx.close()


# ---- cs_column_batch ----------------------------------------------------------------------------------------------------------------

NP_COL = 31                                   # Discretized(5, 2): K = 31 node states per profile


def _profiles(cs, P, B, seed):
    rng = np.random.default_rng(seed)
    T0 = np.clip(W.earth_temperature(P), 190.0, 320.0)
    return [np.clip(T0 + rng.uniform(-6.0, 6.0) + rng.uniform(-2.0, 2.0, len(P)), 180.0, 330.0) for _ in range(B)]


def _straddling(K, B, b0):
    """the profiles holding the states on both sides of every boundary, and the first and last"""
    return sorted({0, B - 1} | {k // K for k0 in b0 for k in (k0 - 1, k0)})


def _batch_vs_single(col, Ts, picks, tol):
    Bu, Bd = col.run_batch(Ts, 0.029)
    for b in picks:
        col.update(Ts[b], 0.029)
        col.run()
        Fu, Fd = col.fetch()
        fm = np.max(Fu)
        assert np.max(np.abs(Bu[b] - Fu)) < tol * fm and np.max(np.abs(Bd[b] - Fd)) < tol * fm, (b, np.max(np.abs(Bu[b] - Fu)) / fm)
    return Bu, Bd


# (shape code, cut-off) of the one-gas columns
COLUMN_CASES = [(0, 25.0), (3, 25.0), (4, 5.0), (5, 25.0), (6, 25.0)]


@pytest.mark.parametrize("code,cut", COLUMN_CASES, ids=[f"code{c}" for c, _ in COLUMN_CASES])
def test_column_batch(cs, O, big, code, cut):
    """B x K >= 2 kc + 1 states of one gas: the straddling, first and last profiles against single runs at 5e-13; one straddling profile
    against the oracle column at 1e-11 (codes 4-6 as sigma_extra = C x sigma at every node)"""
    sl = big["CO2" if code == 3 else "H2O"]
    nu = GRID_CO2 if code == 3 else GRID
    ped = code in (4, 6)
    K = NP_COL
    B = states_for("column", NLINES, len(nu), step=K, ped=ped) // K
    kc, b0 = boundaries("column", B * K, NLINES, len(nu), ped=ped)
    assert any(k0 % K for k0 in b0)                         # a profile's states straddle a boundary
    ctx = cs.Context(0)
    P = cs.pressuregrid(10.0, 1e5, NP_COL)
    Ts = _profiles(cs, P, B, code)
    conc = 400e-6 if code == 3 else (lambda T, P_: 1e-3 * (T / 250.0) ** 2)
    gas = cs.DirectGas(sl, conc, nu, shape=SHAPE_NAMES[code], dnu_cut=cut)
    col = cs.Column(P, 9.8, Ts[0], 0.029, 0.0, 0.0, gas, core=cs.Discretized(5, 2), ctx=ctx)
    assert col.K == K
    picks = _straddling(K, B, b0)
    _batch_vs_single(col, Ts, picks, 5e-13)
    # the oracle at a straddling profile (col holds the last pick; re-run one that straddles)
    b = next(k0 // K for k0 in b0 if k0 % K)
    col.update(Ts[b], 0.029)
    col.run()
    Fu, Fd = col.fetch()
    sub = _reach(sl, nu, cut)
    if code in FLAGS:
        extra = np.zeros((K, len(nu)))
        for k in range(K):
            Ck = col.conc[0, k]
            extra[k] = Ck * X.expected(cs, O, sub, nu, col.Tk[k], col.Pk[k], Ck * col.Pk[k], cut=cut, strict=False, **FLAGS[code])[0]
        ref = O.fluxes_discretized(nu, col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [], [], [], np.zeros((0, K)), sigma_extra=extra,
                                   theta_s=col.theta_s, nstream=col.core.nstream)
    else:
        ref = O.fluxes_discretized(nu, col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [sub], [SHAPE_NAMES[code]], [cut], col.conc,
                                   theta_s=col.theta_s, nstream=col.core.nstream)
    fm = np.max(ref["Fup"])
    assert np.max(np.abs(Fu - ref["Fup"])) < 1e-11 * fm and np.max(np.abs(Fd - ref["Fdn"])) < 1e-11 * fm
    ctx.close()


def test_column_batch_everything(cs, big):
    """every member a batch can hold, across chunk boundaries: a merged code-0 group of two gases (concentrations at stride B K), a
    code-5 and a code-6 group (the second code-5/6 group sums into its own plane), a baked Gas, a CIA pair and a gray term"""
    nu = 1.5 + 0.1 * np.arange(400)            # inside the CIA bands (1-750 cm^-1); lines below 23.5 cm^-1 reach the mirror terms
    K = NP_COL
    L = NLINES                                  # the largest group: the 400 000-line table
    B = states_for("column", L, len(nu), step=K, ped=True, vvh2=True) // K
    kc, b0 = boundaries("column", B * K, L, len(nu), ped=True, vvh2=True)
    assert any(k0 % K for k0 in b0)
    ctx = cs.Context(0)
    P = cs.pressuregrid(10.0, 1e5, NP_COL)
    Ts = _profiles(cs, P, B, 21)
    Om = cs.AtmosphericDomain((170.0, 340.0), 8, (5.0, 1.2e5), 10)
    co2 = cs.DirectGas(cs.SpectralLines.synthetic(2, 3000, 31, 0.0, 200.0), lambda T, P_: 0.3 * (T / 250.0), nu)
    ch4 = cs.DirectGas(cs.SpectralLines.synthetic(6, 3000, 32, 0.0, 200.0), lambda T, P_: 0.01 * (250.0 / T), nu)
    h5 = cs.DirectGas(big["H2O"], lambda T, P_: 1e-3 * (T / 250.0) ** 2, nu, shape="voigtVVH")
    h6 = cs.DirectGas(big["H2O"], lambda T, P_: 2e-3 * (T / 250.0), nu, shape="voigtCKDVVH", dnu_cut=5.0)
    baked = cs.Gas(cs.SpectralLines(os.path.join(HITRAN, "H2O.par"), numin=0.0, numax=150.0), 0.005, nu, Om, ctx=ctx)
    x1 = cs.CIATables(W.fixture("CO2-CO2_2018.cia"))
    col = cs.Column(P, 9.8, Ts[0], 0.029, 0.0, 0.0, co2, ch4, h5, h6, baked, x1, cs.GrayGas(1e-28, nu), core=cs.Discretized(5, 2),
                    ctx=ctx)
    _batch_vs_single(col, Ts, _straddling(K, B, b0), 5e-13)
    info = col.info()
    assert info["groups"] == 3 and info["max_members"] == 2, info     # {co2, ch4} merged; code 5; code 6
    ctx.close()


def test_column_batch_mixed(cs, big):
    """mixed precision (fp32 far-wing records: 16 more bytes per line and state): the batch against sequential mixed runs at the
    tolerance of test_mixed_precision_variant.  far_s = 1e6 is the smallest cs_set_precision accepts (the most far wings in fp32)"""
    sl, nu = big["H2O"], GRID
    K = NP_COL
    B = states_for("column", NLINES, len(nu), step=K, mixed=True) // K
    kc, b0 = boundaries("column", B * K, NLINES, len(nu), mixed=True)
    assert kc < chunk_size("column", B * K, NLINES, len(nu))          # the fp32 records shrink the chunk
    ctx = cs.Context(0)
    ctx.set_precision("mixed", 1e6)
    P = cs.pressuregrid(10.0, 1e5, NP_COL)
    Ts = _profiles(cs, P, B, 41)
    col = cs.Column(P, 9.8, Ts[0], 0.029, 0.0, 0.0, cs.DirectGas(sl, lambda T, P_: 1e-3 * (T / 250.0) ** 2, nu), core=cs.Discretized(5, 2),
                    ctx=ctx)
    _batch_vs_single(col, Ts, _straddling(K, B, b0), 1e-6)
    ctx.close()


# ---- the 65535 cap on gridDim.y -----------------------------------------------------------------------------------------------------

N_CAP = 65552                                     # 65535 + 17: the last chunk holds 17 states


@pytest.mark.parametrize("code", [0, 6])
def test_shape_batch_grid_y_cap(cs, O, code):
    sl = cs.SpectralLines.synthetic(1, 20, 5, 0.0, 12.0)
    nu = 0.5 + 0.125 * np.arange(64)
    cut = 25.0
    kc = chunk_size("shape", N_CAP, 20, len(nu), ped=code == 6)
    assert kc == GRID_Y and N_CAP - kc == 17
    T, P, Pp = _states(N_CAP, 50 + code)
    ctx = cs.Context(0)
    s = cs.shape_batch(sl, code, nu, T, P, Pp, cut, ctx)
    small = np.concatenate([cs.shape_batch(sl, code, nu, T[a:a + 4096], P[a:a + 4096], Pp[a:a + 4096], cut, ctx) for a in range(0, N_CAP, 4096)])
    _close_rows(s, small)
    for k in (0, 1, 4095, 4096, kc - 1, kc, N_CAP - 1):
        assert _vs_ref(s[k], _ref(cs, O, sl, code, nu, T[k], P[k], Pp[k], cut, True), code) < 1e-11, k
    ctx.close()


def test_bake_grid_y_cap(cs, O):
    sl = cs.SpectralLines.synthetic(1, 20, 6, 0.0, 12.0)
    nu = 0.5 + 0.125 * np.arange(64)
    nT, nP = 241, 272
    n = nT * nP
    assert n == N_CAP and chunk_size("bake", n, 20, len(nu)) == GRID_Y
    ctx = cs.Context(0)
    Om = cs.AtmosphericDomain((170.0, 330.0), nT, (10.0, 1e5), nP)
    g = cs.Gas(sl, 0.01, nu, Om, ctx=ctx, keep_host_tables=True)
    Z = g.lnsigma
    TT, PP = np.meshgrid(Om.T, Om.P, indexing="ij")
    Tf, Pf = TT.ravel(order="F"), PP.ravel(order="F")
    s = np.concatenate([cs.shape_batch(sl, 0, nu, Tf[a:a + 4096], Pf[a:a + 4096], 0.01 * Pf[a:a + 4096], 25.0, ctx) for a in range(0, n, 4096)])
    assert np.all(s > 0)
    ref = np.log(s).T.reshape(len(nu), nT, nP, order="F")
    assert np.max(np.abs(Z - ref)) < 1e-12 * np.max(np.abs(ref))
    for k in (0, GRID_Y - 1, GRID_Y, n - 1):
        i, j = k % nT, k // nT
        r = O.shape_bang("voigt", nu, sl, Om.T[i], Om.P[j], 0.01 * Om.P[j], 25.0)
        assert relerr(np.exp(Z[:, i, j]), r) < 1e-11, k
    ctx.close()


# ---- pressure-shifted line centres: CS_SHAPE_PSHIFT on codes 0-2, and code 7 --------------------------------------------------------
#
# Who is inside a cut-off depends on the state here (c = nul + delta_a P / P0), so a chunk has state-dependent pieces of its own: the
# records parked per state by the strict pre-filter, the windows and zones widened ONCE by the largest shift ds of ALL K states, the
# per-state fringe tests of the pedestal finish -- each indexed by the chunk-local state, with the pressures at p.Pk = dP + k0.

GRID_DY = 0.5 + 0.125 * np.arange(400)       # dyadic, 0.5 .. 50.375 cm^-1: nu - s, nu + s and nu + c are exact in fp64
SHIFT_SEED = 13
SHIFT_CASES = [(0 | PSHIFT, 25.0), (1 | PSHIFT, 5.0), (2 | PSHIFT, 25.0), (7, 5.0), (7, 25.0), (7, 0.25)]   # 0.25 < the largest shift, 0.375
SHIFT_IDS = [f"code{c & ~PSHIFT}{'-shifted' if c & PSHIFT else ''}-cut{u:g}" for c, u in SHIFT_CASES]
BAKE_SHIFT_CASES = [0 | PSHIFT, 7]
COLUMN_SHIFT_CASES = [(0 | PSHIFT, 5.0), (7, 5.0)]
NT_BAKE = 17
_SHIFTED = {}


def shifted_lines():
    """The arrays of the shifted table: up to 400 000 lines (the distinct ones of 400 000 draws) at multiples of 2^-6 over 0-25 000 cm^-1,
    delta_a from voigt_lbl_ref.DELTAS (multiples of 2^-5) with the sign alternating along runs of neighbours, as in voigt_lbl_ref.case_table:
    neighbours swap their order under pressure.  nu and delta_a are what the .par file's fields hold exactly."""
    if not _SHIFTED:
        rng = np.random.default_rng(SHIFT_SEED)
        # (as in case_table, a pair of lines 2^-4 on either side of every limit the strict pre-filter sets on GRID_DY, shifting towards it:
        # the lower one reaches the limit exactly at 0.5 atm, the upper one crosses it above 1/3 atm)
        edge = {int(round((lim + off) * 64)): d for D in (0.25, 5.0, 25.0) for lim in (GRID_DY[0] - D, GRID_DY[-1] + D) if lim > 0.0625
                for off, d in ((-0.0625, 0.125), (0.0625, -0.1875))}
        q = np.unique(np.concatenate([rng.integers(1, 25000 * 64, NLINES), list(edge)]))
        nul = q / 64.0
        n = len(nul)
        da = rng.choice(V.DELTAS, n)
        alt = rng.random(n) < 0.5
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        da = np.round(np.where(alt, np.clip(np.abs(da) * sign, V.DELTAS[0], V.DELTAS[-1]), da) * 32.0) / 32.0
        da[np.searchsorted(q, list(edge))] = list(edge.values())
        _SHIFTED.update(nu=nul, S=10.0 ** rng.uniform(-24, -19, n), gamma_a=np.round(rng.uniform(0.05, 0.10, n), 4),
                        gamma_s=np.round(rng.uniform(0.2, 0.5, n), 3), Epp=np.round(rng.uniform(0, 2000, n), 4),
                        na=np.round(rng.uniform(0.6, 0.8, n), 2), delta_a=da)
    return _SHIFTED


@pytest.fixture(scope="module")
def shifted(cs, tmp_path_factory):
    """the shifted table through a .par file: the only way a slot gets shifts"""
    t = shifted_lines()
    path = os.path.join(str(tmp_path_factory.mktemp("chunks")), "shifted.par")
    sl = cs.SpectralLines(PS.write_par(path, 1, t["nu"], t["S"], t["gamma_a"], t["gamma_s"], t["Epp"], t["na"], t["delta_a"]))
    assert np.array_equal(sl.nu, t["nu"]) and np.array_equal(sl.delta_a, t["delta_a"])
    return sl


def shifted_states(n, kc, seed):
    """(T, P, Pp) of n states: P = P0 r / 16, r = 1 .. 32 (dyadic multiples of P0 up to 2 atm).  The first chunk stays at or below 0.5 atm
    (its first row holds 0.125 atm, its last 0.5 atm) and the first row of every later chunk holds 2 atm: the largest shift ds belongs
    to no state of the first chunk, and the compared rows on the two sides of a boundary differ most."""
    rng = np.random.default_rng(seed)
    T = rng.uniform(180.0, 330.0, n)
    r = rng.integers(1, 33, n)
    r[:kc] = rng.integers(1, 9, kc)
    r[0], r[kc - 1] = 2, 8
    r[kc::kc] = 32
    P = KATM * r / 16.0
    return T, P, P * 10.0 ** rng.uniform(-4.0, -1.3, n)


class _Case:
    pass


def shift_case(code, cut):
    """sizes, states and compared rows of one shifted shape case (no GPU: test_state_chunk_rules.py holds them to their premises)"""
    L, ped = len(shifted_lines()["nu"]), code == 7
    c = _Case()
    c.n = states_for("shape", L, len(GRID_DY), ped=ped)
    c.kc, c.b0 = boundaries("shape", c.n, L, len(GRID_DY), ped=ped)
    c.T, c.P, c.Pp = shifted_states(c.n, c.kc, 300 + code + int(cut))
    # (one code-7 reference row at cut 25 costs what fifteen cost at cut 5: the boundary, first and last rows only)
    c.rows = sorted({0, c.n - 1} | {k for k0 in c.b0 for k in (k0 - 1, k0)}) if (code, cut) == (7, 25.0) else _check_rows(c.n, c.b0, code)
    return c


def bake_sizes(code):
    """(nP, n, kc, b0) of a shifted bake of NT_BAKE x nP knots"""
    L, ped = len(shifted_lines()["nu"]), code == 7
    nP = -(-states_for("bake", L, len(GRID_DY), step=NT_BAKE, ped=ped) // NT_BAKE)
    return (nP, NT_BAKE * nP) + boundaries("bake", NT_BAKE * nP, L, len(GRID_DY), ped=ped)


def column_sizes(code, **kw):
    """(B, kc, b0) of a shifted column batch"""
    L, ped = len(shifted_lines()["nu"]), code == 7
    B = states_for("column", L, len(GRID_DY), step=NP_COL, ped=ped, **kw) // NP_COL
    return (B,) + boundaries("column", B * NP_COL, L, len(GRID_DY), ped=ped, **kw)


def _call(fn, sl, code, nu, T, P, Pp, cut, ctx):
    return fn(sl, SHAPE_NAMES[code & ~PSHIFT], nu, T, P, Pp, cut, ctx, pressure_shift=bool(code & PSHIFT))


def _shift_ref(cs, O, sub, code, nu, T, P, Pp, cut, strict):
    """(value, scale) of one state: voigt_lbl_ref.expected for code 7 (scale: R x the magnitudes of the parts), test_gpu_pressure_shift's
    for the flagged codes (scale: the row's largest value, as that module measures)"""
    if code == 7:
        return V.expected(cs, O, sub, sub.delta_a, nu, T, P, Pp, cut, strict)
    r = PS.expected(O, sub, sub.delta_a, SHAPE_NAMES[code & ~PSHIFT], nu, T, P, Pp, strict, cut)
    return r, np.full(len(nu), np.max(np.abs(r)))


def _unshifted(code):
    """the code without the shift: the base code of a flagged one, code 6 for code 7"""
    return 6 if code == 7 else code & ~PSHIFT


def _moved(a, b, code):
    """the shift is no rounding matter: more than 1e-6 at more than half the points (test_b1_exact_shifts_and_edges).  The Doppler cores,
    1e-4 cm^-1 wide, are exact zeros at all but the grid points a centre sits on, so there: another set of values"""
    return not np.array_equal(a, b) if code & ~PSHIFT == 2 else np.mean(np.abs(a - b) > 1e-6 * b) > 0.5


@pytest.mark.parametrize("code,cut", SHIFT_CASES, ids=SHIFT_IDS)
def test_shifted_shape_batch_and_points(cs, O, shifted, ctxs, code, cut):
    """test_shape_batch_and_points on the shifted table at dyadic pressures: the whole result against calls of fewer than kc states at
    5e-13, the compared rows against the reference at the exact-shift bar of 1e-11 (Doppler 1e-9)"""
    sl, nu = shifted, GRID_DY
    c = shift_case(code, cut)
    assert c.kc == chunk_size("shape", c.n, len(sl.nu), len(nu), ped=code == 7) and np.max(c.P[:c.kc]) < np.max(c.P)
    T, P, Pp = c.T, c.P, c.Pp
    sub = _reach(sl, nu, cut)
    V.dyadic_premise(sub.nu, nu, sub.delta_a, np.unique(P[c.rows]))
    tol = 1e-9 if code & ~PSHIFT == 2 else 1e-11
    worst = 0.0
    for fn, strict in ((cs.shape_batch, True), (cs.shape_points, False)):
        refs = {k: _shift_ref(cs, O, sub, code, nu, T[k], P[k], Pp[k], cut, strict) for k in c.rows}
        for on, ctx in ctxs.items():
            s = _call(fn, sl, code, nu, T, P, Pp, cut, ctx)
            assert s.shape == (c.n, len(nu))
            small = _pieces(lambda a, b: _call(fn, sl, code, nu, T[a:b], P[a:b], Pp[a:b], cut, ctx), c.n, c.kc)
            _close_rows(s, small)
            for k in c.rows:
                e = X.err(s[k], refs[k])
                worst = max(worst, e)
                assert e < tol, (fn.__name__, on, k, e)
        hi = [k for k in c.rows if P[k] >= 0.25 * KATM]
        s0 = fn(sl, SHAPE_NAMES[_unshifted(code)], nu, T[hi], P[hi], Pp[hi], cut, ctxs[True])
        assert len(hi) >= 4 and all(_moved(s[k], s0[i], code) for i, k in enumerate(hi)), fn.__name__
    print(f"code {code} cut {cut}: {c.n} states in chunks of {c.kc}, {len(c.rows)} reference rows, worst error {worst:.2e}")


def test_ld_state_padding_shifted(cs, O, shifted, ctxs):
    """test_ld_state_padding on code 7"""
    sl, nu, cut, code = shifted, GRID_DY, 5.0, 7
    c = shift_case(code, cut)
    T, P, Pp = c.T, c.P, c.Pp
    ctx = ctxs[True]
    ld = len(nu) + 37
    out = np.full((c.n, ld), np.nan)
    cs.check(cs.lib().cs_shape_batch(ctx.handle, ctx.slot_of(sl, shift=True), code, cut, len(nu), cs.dptr(nu), c.n, cs.dptr(T), cs.dptr(P),
                                     cs.dptr(Pp), cs.dptr(out), ld))
    assert np.all(np.isnan(out[:, len(nu):]))
    _close_rows(out[:, :len(nu)], _pieces(lambda a, b: cs.shape_batch(sl, code, nu, T[a:b], P[a:b], Pp[a:b], cut, ctx), c.n, c.kc))
    sub = _reach(sl, nu, cut)
    worst = max(X.err(out[k, :len(nu)], _shift_ref(cs, O, sub, code, nu, T[k], P[k], Pp[k], cut, True))
                for k in (c.b0[0] - 1, c.b0[0], c.b0[-1] - 1, c.b0[-1], c.n - 1))
    print(f"ld_state padding, code 7: worst error {worst:.2e}")
    assert worst < 1e-11


@pytest.mark.parametrize("code", BAKE_SHIFT_CASES, ids=["code0-shifted", "code7"])
def test_bake_shifted(cs, O, shifted, code):
    """test_bake on the shifted table, P knots up to 2 atm (ascending: the largest shift belongs to the last chunk).  The knots are
    no dyadic multiples of P0, so the reference is held at the 1e-9 of arbitrary pressures (tests/test_gpu_voigt_lbl.py's docstring)"""
    sl, nu, cut = shifted, GRID_DY, 5.0
    nT = NT_BAKE
    nP, n, kc, b0 = bake_sizes(code)
    assert kc == chunk_size("bake", n, len(sl.nu), len(nu), ped=code == 7)
    ctx = cs.Context(0)
    Om = cs.AtmosphericDomain((170.0, 330.0), nT, (10.0, 2.0 * KATM), nP)
    g = cs.Gas(sl, 0.01, nu, Om, shape=SHAPE_NAMES[code & ~PSHIFT], dnu_cut=cut, ctx=ctx, keep_host_tables=True,
               pressure_shift=bool(code & PSHIFT))
    Z = g.lnsigma
    assert Z.shape == (len(nu), nT, nP) and not np.any(np.isnan(Z))
    TT, PP = np.meshgrid(Om.T, Om.P, indexing="ij")
    Tf, Pf = TT.ravel(order="F"), PP.ravel(order="F")
    assert np.max(Pf[:kc]) < 0.5 * np.max(Pf)
    s = _pieces(lambda a, b: _call(cs.shape_batch, sl, code, nu, Tf[a:b], Pf[a:b], 0.01 * Pf[a:b], cut, ctx), n, kc)
    flat = s.T.reshape(len(nu), nT, nP, order="F")
    tiny = np.finfo(float).tiny
    z = (flat.reshape(len(nu), -1).min(axis=1) == 0) & (flat.reshape(len(nu), -1).max(axis=1) > 0)
    flat[z] = 0.0
    with np.errstate(divide="ignore"):
        ref = np.where(np.all(flat <= tiny, axis=(1, 2))[:, None, None], np.log(tiny), np.log(flat))
    assert np.array_equal(np.isfinite(Z), np.isfinite(ref))
    m = np.isfinite(ref) & (ref > np.log(tiny))
    assert np.max(np.abs(Z[m] - ref[m])) < 1e-12 * np.max(np.abs(ref[m]))
    sub = _reach(sl, nu, cut)
    worst = 0.0
    for k in sorted({0, n - 1} | {k for k0 in b0 for k in (k0 - 1, k0)}):
        i, j = k % nT, k // nT
        r = _shift_ref(cs, O, sub, code, nu, Om.T[i], Om.P[j], 0.01 * Om.P[j], cut, True)
        with np.errstate(divide="ignore"):
            e = X.err(np.exp(Z[:, i, j]) * (Z[:, i, j] > np.log(tiny)), r)
        worst = max(worst, e)
        assert e < 1e-9, (k, e)
    print(f"bake, code {code}: {n} knots in chunks of {kc}, worst error {worst:.2e}")
    ctx.close()


@pytest.mark.parametrize("code,cut", COLUMN_SHIFT_CASES, ids=["code0-shifted", "code7"])
def test_column_batch_shifted(cs, O, shifted, code, cut):
    """test_column_batch on the shifted table: batch against single runs at 5e-13; one straddling profile against the oracle column with
    C x sigma as sigma_extra at 1e-9 (node pressures are arbitrary: tests/test_gpu_voigt_lbl.py's docstring)"""
    sl, nu, K = shifted, GRID_DY, NP_COL
    B, kc, b0 = column_sizes(code)
    assert kc == chunk_size("column", B * K, len(sl.nu), len(nu), ped=code == 7) and any(k0 % K for k0 in b0)
    ctx = cs.Context(0)
    P = cs.pressuregrid(10.0, 1e5, NP_COL)
    Ts = _profiles(cs, P, B, code)
    gas = cs.DirectGas(sl, lambda T, P_: 1e-3 * (T / 250.0) ** 2, nu, shape=SHAPE_NAMES[code & ~PSHIFT], dnu_cut=cut,
                       pressure_shift=bool(code & PSHIFT))
    col = cs.Column(P, 9.8, Ts[0], 0.029, 0.0, 0.0, gas, core=cs.Discretized(5, 2), ctx=ctx)
    assert col.K == K
    _batch_vs_single(col, Ts, _straddling(K, B, b0), 5e-13)
    b = next(k0 // K for k0 in b0 if k0 % K)
    col.update(Ts[b], 0.029)
    col.run()
    Fu, Fd = col.fetch()
    sub = _reach(sl, nu, cut)
    extra = np.zeros((K, len(nu)))
    for k in range(K):
        Ck = col.conc[0, k]
        extra[k] = Ck * _shift_ref(cs, O, sub, code, nu, col.Tk[k], col.Pk[k], Ck * col.Pk[k], cut, False)[0]
    ref = O.fluxes_discretized(nu, col.P, col.g, 2, col.Tn, col.mun, col.Tlev, [], [], [], np.zeros((0, K)), sigma_extra=extra,
                               theta_s=col.theta_s, nstream=col.core.nstream)
    fm = np.max(ref["Fup"])
    e = max(np.max(np.abs(Fu - ref["Fup"])), np.max(np.abs(Fd - ref["Fdn"]))) / fm
    print(f"column batch, code {code}: {B} profiles in chunks of {kc} states, worst flux error {e:.2e}")
    assert e < 1e-9
    # the unshifted code would miss that bar: the comparison above sees the shifts
    col0 = cs.Column(P, 9.8, Ts[b], 0.029, 0.0, 0.0, cs.DirectGas(sl, gas.fC, nu, shape=SHAPE_NAMES[_unshifted(code)], dnu_cut=cut),
                     core=cs.Discretized(5, 2), ctx=ctx)
    col0.run()
    moved = np.max(np.abs(col0.fetch()[0] - Fu)) / fm
    print(f"column batch, code {code}: the shifts move the flux by {moved:.2e}")
    assert moved > 100 * 1e-9
    ctx.close()


def test_column_batch_everything_shifted(cs, shifted):
    """every shifted member beside the unshifted ones, across chunk boundaries: a code-5, a code-6 and a code-7 group on one table (three
    code-5/6/7 groups: the second and the third sum into the one spare plane, one after the other), a flagged code-0 group, a baked
    code-7 Gas, a CIA pair with its unflagged CO2 lines and a gray term"""
    nu = 1.5 + 0.125 * np.arange(400)          # inside the CIA bands (1-750 cm^-1); lines below 23.5 cm^-1 reach the mirror terms
    K = NP_COL
    B, kc, b0 = column_sizes(7, vvh2=True)
    assert kc == chunk_size("column", B * K, len(shifted.nu), len(nu), ped=True, vvh2=True) and any(k0 % K for k0 in b0)
    ctx = cs.Context(0)
    P = cs.pressuregrid(10.0, 1e5, NP_COL)
    Ts = _profiles(cs, P, B, 22)
    Om = cs.AtmosphericDomain((170.0, 340.0), 8, (5.0, 1.2e5), 10)
    h5 = cs.DirectGas(shifted, lambda T, P_: 1e-3 * (T / 250.0) ** 2, nu, shape="voigtVVH")
    h6 = cs.DirectGas(shifted, lambda T, P_: 2e-3 * (T / 250.0), nu, shape="voigtCKDVVH", dnu_cut=5.0)
    h7 = cs.DirectGas(shifted, lambda T, P_: 1.5e-3 * (250.0 / T), nu, shape="voigtLBL", dnu_cut=5.0)
    h0 = cs.DirectGas(shifted, lambda T, P_: 5e-4 * (T / 250.0), nu, dnu_cut=5.0, pressure_shift=True)
    co2 = cs.DirectGas(cs.SpectralLines.synthetic(2, 3000, 31, 0.0, 200.0), lambda T, P_: 0.3 * (T / 250.0), nu)   # (the CIA pair's gas)
    baked = cs.Gas(cs.SpectralLines(os.path.join(HITRAN, "H2O.par"), numin=0.0, numax=150.0), 0.005, nu, Om, shape="voigtLBL", ctx=ctx)
    x1 = cs.CIATables(W.fixture("CO2-CO2_2018.cia"))
    col = cs.Column(P, 9.8, Ts[0], 0.029, 0.0, 0.0, h5, h6, h7, h0, co2, baked, x1, cs.GrayGas(1e-28, nu), core=cs.Discretized(5, 2),
                    ctx=ctx)
    _batch_vs_single(col, Ts, _straddling(K, B, b0), 5e-13)
    info = col.info()
    assert info["groups"] == 5 and info["max_members"] == 1, info     # codes 5, 6, 7, 0 | 16 and 0: no two merge
    ctx.close()
