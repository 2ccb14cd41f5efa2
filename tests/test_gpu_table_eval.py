"""Opacity tables and the accelerated absorber on synthetic knot values uploaded directly (cs_table_upload, cs_accel_upload): no line sums,
so the reference is 40-digit interpolation of numbers the test chose (tests/tabulated_ref.py) and the tolerance is derived:
|d exponent| <= (M + 4 (nT + nP) + 8) 2^-53 sum_m |Z_m| |W_m| for k_table_eval_mfma's M = nT nP term contraction, + 4 ulp on sigma,
asserted element-wise with factor 1.  Z = f(nu) + g(iT) + h(iP) + a cross term in [-120, -40] with nT != nP in most cases and g != h: a
transposed index, a dropped table node or a shifted state column is a percent-level error.

The product of the grids (nT, nP), the state counts K and the wavenumber counts nnu below is covered pairwise: every value of each axis meets every value of each other axis at least
once (_cases: 7 grids x 8 K x 7 nnu in 56 columns instead of 392), plus cs_table_eval (K = 1) on every grid and nnu.
Each test prints its largest error / bound ratio (pytest -s)."""
import ctypes as C
import math

import numpy as np
import pytest

import tabulated_ref as R

pytestmark = pytest.mark.gpu

GRIDS = [(2, 2), (2, 3), (3, 3), (3, 5), (5, 5), (8, 12), (12, 24)]              # M % 4 = 0, 2, 1, 3, 1, 0, 0
KS = {15: (15, 2), 16: (6, 4), 17: (9, 3), 31: (16, 3), 32: (32, 2), 33: (17, 3), 63: (32, 3), 65: (33, 3)}     # K -> (np, nlobatto)
NNUS = [1, 63, 64, 65, 255, 257, 1025]
TR, PR = (150.0, 420.0), (3.0, 2e5)


def _cases():
    """every (grid, K), (grid, nnu) and (K, nnu) pair at least once: 7 x 8 rows, the nnu axis rotated against both others"""
    out = []
    ks = sorted(KS)
    for gi, g in enumerate(GRIDS):
        for ki, K in enumerate(ks):
            out.append((g, K, NNUS[(gi + ki) % 7]))
    pairs = {(K, n) for _, K, n in out}
    for K in ks:                                    # 8 K x 7 nnu needs 56 rows and the rotation gives each (K, nnu) once: complete
        for n in NNUS:
            assert (K, n) in pairs
    return out


@pytest.fixture(scope="module")
def ctx(cs):
    c = cs.Context(0)
    yield c
    c.close()


def _upload(cs, ctx, slot, nu, Om, Z, order="C"):
    """Z[nnu, nT, nP]: the header's column-major [nnu, nT, nP] (nu fastest) == C-ordered [nP][nT][nnu]"""
    if order == "C":
        buf = np.ascontiguousarray(np.transpose(Z, (2, 1, 0)))
    else:
        buf = np.asfortranarray(Z)
    ptr = buf.ctypes.data_as(C.POINTER(C.c_double))
    return cs.lib().cs_table_upload(ctx.handle, slot, len(nu), cs.dptr(cs.as_f64(nu)), Om.nT, cs.dptr(cs.as_f64(Om.T)), Om.nP, cs.dptr(cs.as_f64(Om.P)), ptr)


def _eval(cs, ctx, slot, T, P, i0, n):
    out = np.zeros(n)
    rc = cs.lib().cs_table_eval(ctx.handle, slot, float(T), float(P), i0, n, cs.dptr(out))
    return rc, out


def _table_gas(cs, ctx, lines, nu, Om, Z, conc, name="CO2"):
    """cs.Gas bakes; to put an uploaded table under a Column, a small baked Gas gives the slot and the upload replaces its contents"""
    g = cs.Gas(lines(name), conc, nu, Om, ctx=ctx)
    cs.check(_upload(cs, ctx, g.slot, nu, Om, Z))
    return g


def _ratio(a, ref, bound):
    return float(np.max(np.abs(a - ref) / ref / bound))


def _column_ref(col, tabs):
    """sum_t conc_t sigma_t at the node states + the bound of the sum (each term's own bound on its own share)"""
    sig, err = np.zeros((col.K, col.nnu)), np.zeros((col.K, col.nnu))
    for (Om, Z, conc) in tabs:
        for k in range(col.K):
            s, A = R.table_sigma(Z, Om.T, Om.P, col.Tk[k], col.Pk[k])
            c = conc(col.Tk[k], col.Pk[k]) if callable(conc) else conc
            sig[k] += c * s
            err[k] += c * s * (R.table_bound(Om.nT, Om.nP, A) + 2 * R.U)
    return sig, err


@pytest.mark.parametrize("nTP", GRIDS)
def test_table_eval_points(cs, ctx, nTP):
    """cs_table_eval (K = 1) on every grid and wavenumber count: on a knot conc exp(Z_knot) to the ulps of exp, one ulp off a knot, both
    pressure ends, inside the 1e-12 slack (clamped) and beyond it / one ulp outside in T (CS_EINVAL); sub-ranges bitwise; both layouts"""
    nT, nP = nTP
    Om = cs.AtmosphericDomain(TR, nT, PR, nP)
    worst = 0.0
    for nnu in NNUS:
        nu = R.grid(nnu)
        Z = R.table_values(nu, nT, nP)
        assert _upload(cs, ctx, 3, nu, Om, Z) == 0
        i, j = nT // 2, nP // 3
        rc, s = _eval(cs, ctx, 3, Om.T[i], Om.P[j], 0, nnu)
        ex = np.array([float(R.mp.exp(R.mp.mpf(float(z)))) for z in Z[:, i, j]])
        assert rc == 0 and np.all(np.abs(s - ex) <= 8 * R.U * ex)                     # 4 ulp: the weights are exactly 0 and 1
        pts = [(float(np.nextafter(Om.T[i], Om.T[0] if i == nT - 1 else np.inf)), Om.P[j]), (Om.T[0], Om.P[0]), (Om.T[-1], Om.P[-1]), (233.3, 77.7),
               (Om.T[-1], math.exp(math.log(Om.P[-1]) + 5e-13)), (151.0, math.exp(math.log(Om.P[0]) - 5e-13))]
        for T, P in pts[: (None if nnu in (65, 1025) else 4)]:
            rc, s = _eval(cs, ctx, 3, T, P, 0, nnu)
            ref, A = R.table_sigma(Z, Om.T, Om.P, T, P)
            assert rc == 0
            q = _ratio(s, ref, R.table_bound(nT, nP, A))
            worst = max(worst, q)
            assert q <= 1.0, (nnu, T, P, q)
        assert _eval(cs, ctx, 3, 233.3, math.exp(math.log(Om.P[-1]) + 3e-12), 0, nnu)[0] == -1
        assert _eval(cs, ctx, 3, 233.3, math.exp(math.log(Om.P[0]) - 3e-12), 0, nnu)[0] == -1
        assert _eval(cs, ctx, 3, float(np.nextafter(Om.T[-1], np.inf)), 100.0, 0, nnu)[0] == -1
        assert _eval(cs, ctx, 3, float(np.nextafter(Om.T[0], 0.0)), 100.0, 0, nnu)[0] == -1
        # sub-ranges
        rc, full = _eval(cs, ctx, 3, 233.3, 77.7, 0, nnu)
        for i0, n in ((0, 1), (nnu - 1, 1), (max(0, min(60, nnu - 8)), min(8, nnu)), (0, nnu)):
            rc, part = _eval(cs, ctx, 3, 233.3, 77.7, i0, n)
            assert rc == 0 and np.array_equal(part, full[i0:i0 + n])
        for i0, n in ((-1, 1), (nnu, 1), (0, nnu + 1), (0, 0)):
            assert _eval(cs, ctx, 3, 233.3, 77.7, i0, n)[0] == -1
        # the Fortran-ordered [nnu, nT, nP] array of the header
        assert _upload(cs, ctx, 4, nu, Om, Z, order="F") == 0
        assert np.array_equal(_eval(cs, ctx, 4, 233.3, 77.7, 0, nnu)[1], full)
    print(f"  grid {nTP}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("nTP,K,nnu", _cases())
def test_column_over_one_table(cs, O, ctx, lines, nTP, K, nnu):
    """sigma at the nodes of a column over one uploaded table; for the K = 17 and 33 rows also tau (the nodes' relative bound + the
    nlobatto + 2 roundings of the Lobatto sum, on either side) and the band fluxes (1e-11 of the largest) through the oracle's depth and
    sweeps, with a good share of the layers above the 1e-6 floor"""
    nT, nP = nTP
    np_, nlob = KS[K]
    Om = cs.AtmosphericDomain(TR, nT, PR, nP)
    nu = R.grid(nnu)
    Z = R.table_values(nu, nT, nP, *((-70.0, -40.0) if K in (17, 33) else ()))     # (the rows that compare tau: layer depths above the floor)
    conc = lambda T, P: 0.2 + 0.5 * (P / 1e5) ** 0.3
    g = _table_gas(cs, ctx, lines, nu, Om, Z, conc)                 # (a one-point grid is accepted like any other)
    P = cs.pressuregrid(5.0, 1e5, np_)
    T = np.linspace(160.0, 410.0, np_)
    T[0], T[-1] = Om.T[0], Om.T[-1]                                 # the domain's temperature ends
    col = cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, g, core=cs.Discretized(4, nlob), ctx=ctx, _warn=False)
    assert col.K == K
    col.run()
    assert col.info()["flux_form"] == 0                             # tables force the separate kernels
    sig, err = _column_ref(col, [(Om, Z, conc)])
    s = col.sigma_nodes()
    q = float(np.max(np.abs(s - sig) / err))
    print(f"  {nTP} K {K} nnu {nnu}: largest error / bound {q:.3f}")
    assert q <= 1.0
    if K in (17, 33):
        tau = np.zeros((col.nl, col.nnu), order="F")
        Fup, Fdn = col.fetch(tau)
        ref = O.fluxes_discretized(nu, P, 9.8, nlob, col.Tn, col.mun, col.Tlev, [], [], [], np.zeros((0, col.K)), sigma_extra=sig, nstream=4,
                                   theta_s=col.theta_s)
        assert (ref["tau"] > 1e-6).mean() > 0.3
        tol = np.max(err / sig, axis=0)[None, :] + 2 * (nlob + 2) * R.U
        assert np.all(np.abs(tau - ref["tau"]) <= tol * ref["tau"])
        if nnu > 1:
            assert np.max(np.abs(Fup - ref["Fup"])) < 1e-11 * ref["Fup"].max() and np.max(np.abs(Fdn - ref["Fdn"])) < 1e-11 * ref["Fup"].max()


def test_accumulation_and_mixed_column(cs, O, ctx, lines):
    """1, 2 and CS_MAX_TABLE = 16 tables with different concentrations in one column; then a table + a CIA pair + a line gas + a gray term:
    form 0, sigma against the sum of the references, tau and fluxes through the oracle"""
    nu = R.grid(130)
    P = cs.pressuregrid(5.0, 1e5, 9)
    T = np.linspace(170.0, 400.0, 9)
    c2 = cs.Context(0)
    try:
        tabs, gases = [], []
        for t in range(16):
            nT, nP = GRIDS[t % 6]
            Om = cs.AtmosphericDomain(TR, nT, PR, nP)
            Z = R.table_values(nu + 0.25 * t, nT, nP, lo=-110.0 + t, hi=-50.0 + t)
            conc = (lambda T_, P_, t=t: 0.01 * (t + 1) * (P_ / 1e5) ** 0.1)
            gases.append(_table_gas(cs, c2, lines, nu, Om, Z, conc))
            tabs.append((Om, Z, conc))
        for n in (1, 2, 16):
            col = cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, *gases[:n], core=cs.Discretized(4, 3), ctx=c2, _warn=False)
            col.run()
            assert col.info()["flux_form"] == 0
            sig, err = _column_ref(col, tabs[:n])
            q = float(np.max(np.abs(col.sigma_nodes() - sig) / (err + n * R.U * sig)))
            print(f"  {n} tables: largest error / bound {q:.3f}")
            assert q <= 1.0
        # a table + a CIA pair + a line gas + a gray term (the line gas sees no line up here: its share is exactly zero)
        data = R.overlap_set(3)
        co2 = cs.DirectGas(lines("CO2"), 0.9, nu)
        gray = cs.GrayGas(3e-26, nu)
        tab = _table_gas(cs, ctx, lines, nu, tabs[3][0], tabs[3][1], tabs[3][2], name="CH4")     # (a second CO2 gas would break the pairing)
        col = cs.Column(P, 9.8, T, 0.044, 0.0, 0.0, co2, tab, gray, cs.CIATables(data), core=cs.Discretized(4, 3), ctx=ctx, _warn=False)
        col.run()
        tau = np.zeros((col.nl, col.nnu), order="F")
        Fup, Fdn = col.fetch(tau)
        assert col.info()["flux_form"] == 0
        sig, err = _column_ref(col, [tabs[3]])
        cia = np.array([R.cia_sigma(data, nu, col.Tk[k], col.Pk[k], col.cia_P1[0, k], col.cia_P2[0, k]) for k in range(col.K)])
        tot = sig + cia + 3e-26
        tol = err + 4 * R.cia_bound(data) * cia + 4 * R.U * tot
        assert np.all(np.abs(col.sigma_nodes() - tot) <= tol)
        ref = O.fluxes_discretized(nu, P, 9.8, 3, col.Tn, col.mun, col.Tlev, [co2.sl], ["voigt"], [25.0], col.conc, sigma_extra=tot, nstream=4,
                                   theta_s=col.theta_s)
        assert np.max(np.abs(tau - ref["tau"]) / ref["tau"]) <= float(np.max(tol / tot)) + 7 * R.U
        assert np.max(np.abs(Fup - ref["Fup"])) < 1e-11 * ref["Fup"].max() and np.max(np.abs(Fdn - ref["Fdn"])) < 1e-11 * ref["Fup"].max()
    finally:
        c2.close()


def test_floatmin_rows_and_cancellation(cs, ctx):
    """rows of ln(floatmin) next to ordinary rows; a table 600 apart between its pressure ends (weights of alternating sign cancel)"""
    nT, nP = 5, 8
    Om = cs.AtmosphericDomain(TR, nT, PR, nP)
    nu = R.grid(70)
    Z = R.table_values(nu, nT, nP)
    Z[::3] = math.log(np.finfo(float).tiny)
    Z2 = R.table_values(nu, nT, nP) - 40.0 + np.linspace(-560.0, 40.0, nP)[None, None, :]
    for Zt in (Z, Z2):
        assert _upload(cs, ctx, 5, nu, Om, Zt) == 0
        for T, P in ((200.2, 5.0), (333.0, 1.5e5), (419.0, 800.0)):
            rc, s = _eval(cs, ctx, 5, T, P, 0, len(nu))
            ref, A = R.table_sigma(Zt, Om.T, Om.P, T, P)
            ok = ref > 1e-300                                       # (a relative bound says nothing about subnormal results)
            assert rc == 0 and ok.any()
            q = _ratio(s[ok], ref[ok], R.table_bound(nT, nP, A)[ok])
            print(f"  largest error / bound {q:.3f}")
            assert q <= 1.0
            assert np.all(s[~ok] <= 1e-299)


@pytest.mark.parametrize("nTP,np_,nlob,B", [((3, 5), 6, 3, 3), ((3, 5), 9, 3, 4), ((8, 12), 9, 3, 2), ((8, 12), 12, 3, 3)])
def test_run_batch_over_tables(cs, O, ctx, lines, nTP, np_, nlob, B):
    """cs_column_batch weights the table at B K states (33, 68, 34, 69: across 32 and 64) through its own code; per profile against the
    reference, one profile touching the domain's temperature end.  A batch returns band fluxes only; the table's values put most layers
    above the optical-depth floor (asserted), so a wrong weight moves them"""
    nT, nP = nTP
    Om = cs.AtmosphericDomain(TR, nT, PR, nP)
    nu = R.grid(129)
    Z = R.table_values(nu, nT, nP, lo=-64.0, hi=-40.0)                # sigma ~ e^-59 .. e^-45: layer depths from below the floor to tens
    g = _table_gas(cs, ctx, lines, nu, Om, Z, 0.3)
    P = cs.pressuregrid(5.0, 1e5, np_)
    col = cs.Column(P, 9.8, np.linspace(200.0, 300.0, np_), 0.029, 0.0, 0.0, g, core=cs.Discretized(4, nlob), ctx=ctx, _warn=False)
    Ts = [np.linspace(160.0 + 20 * b, 330.0 + 20 * b, np_) for b in range(B)]
    Ts[-1][-1] = Om.T[-1]
    Fup, Fdn = col.run_batch(Ts)
    for b, T in enumerate(Ts):
        fT = cs.core.formprofile(P, T)
        Tn, mun = cs.core.lobattoevaluations(P, fT, col._fmu, nlob)
        Tk = cs.core.nodevalues(Tn, nlob)
        sig = np.array([0.3 * R.table_sigma(Z, Om.T, Om.P, Tk[k], col.Pk[k])[0] for k in range(col.K)])
        ref = O.fluxes_discretized(nu, P, 9.8, nlob, Tn, mun, np.array([fT(p) for p in P]), [], [], [], np.zeros((0, col.K)), sigma_extra=sig,
                                   nstream=4, theta_s=col.theta_s)
        share = float((ref["tau"] > 1e-6).mean())
        assert share > 0.5 and ref["tau"].max() > 1.0 and np.median(ref["tau"]) < 10.0, share      # the fluxes depend on the table
        e = max(np.max(np.abs(Fup[b] - ref["Fup"])), np.max(np.abs(Fdn[b] - ref["Fdn"]))) / ref["Fup"].max()
        print(f"  profile {b}: flux err {e:.2e}, layers above the floor {share:.2f}")
        assert e < 1e-11


def test_grid_contract(cs, ctx):
    """cs_table_upload takes Omega.T x Omega.P only: the weights are those of Chebyshev extrema.  AtmosphericDomain grids of every size
    2..24 pass; an ascending grid that is not one is CS_EINVAL, in T and in P"""
    nu = R.grid(10)
    for n in range(2, 25):
        Om = cs.AtmosphericDomain((25.0, 550.0), n, (1.0, 1e6), 26 - n)
        assert np.allclose(Om.T, cs.chebygrid(25.0, 550.0, n)) and np.allclose(np.log(Om.P), cs.chebygrid(0.0, math.log(1e6), 26 - n))
        assert _upload(cs, ctx, 6, nu, Om, R.table_values(nu, n, 26 - n)) == 0
    Om = cs.AtmosphericDomain(TR, 5, PR, 6)
    Z = R.table_values(nu, 5, 6)

    class Other:
        nT, nP, T, P = 5, 6, np.linspace(TR[0], TR[1], 5), Om.P
    assert _upload(cs, ctx, 6, nu, Other, Z) == -1
    Other.T, Other.P = Om.T, np.exp(np.linspace(math.log(PR[0]), math.log(PR[1]), 6))
    assert _upload(cs, ctx, 6, nu, Other, Z) == -1
    Other.P = Om.P.copy()
    Other.P[2] *= 1 + 1e-7
    assert _upload(cs, ctx, 6, nu, Other, Z) == -1
    Other.P = Om.P * (1 + 1e-13)                                         # rounding of exp / log: fine
    assert _upload(cs, ctx, 6, nu, Other, Z) == 0


def test_accelerated_absorber_on_synthetic_knots(cs, O):
    """cs_accel_upload / cs_accel_eval against tabulated_ref.accel_sigma: 2 knots and 11; P on a knot, between, below the first and above
    the last; ln floatmin rows; ragged grids; sub-ranges; a column over the slot with K across 16 and 32.  8 U max|L| + 4 ulp, times the
    extrapolation factor"""
    c = cs.Context(0)
    try:
        for nk, nnu in ((2, 63), (11, 257), (11, 65)):
            nu = R.grid(nnu)
            Pk = np.exp(np.linspace(math.log(20.0), math.log(9e4), nk)) * (1 + 0.01 * np.sin(np.arange(nk)))
            L = -80.0 + 25.0 * np.sin(0.3 * np.arange(nnu)[None, :] + 0.9 * np.arange(nk)[:, None]) + 3.0 * np.arange(nk)[:, None]
            L[:, ::5] = math.log(np.finfo(float).tiny)
            L[0, 2] = math.log(np.finfo(float).tiny)
            cs.check(cs.lib().cs_accel_upload(c.handle, 1, nnu, cs.dptr(nu), nk, cs.dptr(Pk), cs.dptr(np.ascontiguousarray(L))))
            for P in (Pk[0], Pk[-1], Pk[nk // 2], math.sqrt(Pk[0] * Pk[1]), 0.3 * Pk[0], 4.0 * Pk[-1], float(np.nextafter(Pk[-1], 0))):
                out = np.zeros(nnu)
                cs.check(cs.lib().cs_accel_eval(c.handle, 1, float(P), 0, nnu, cs.dptr(out)))
                ref, f = R.accel_sigma(L, Pk, P)
                ok = ref > 1e-290
                assert np.all(np.abs(out[ok] - ref[ok]) <= R.accel_bound(L, f) * ref[ok]), (nk, nnu, P)
                assert np.all(out[~ok] <= 1e-289)
                part = np.zeros(5)
                cs.check(cs.lib().cs_accel_eval(c.handle, 1, float(P), nnu - 5, 5, cs.dptr(part)))
                assert np.array_equal(part, out[-5:])
            assert cs.lib().cs_accel_eval(c.handle, 1, 100.0, nnu - 4, 5, cs.dptr(np.zeros(5))) == -1
        # a column over the slot (65 points): K = 17 and 33
        for np_ in (17, 33):
            P = cs.pressuregrid(30.0, 8e4, np_)
            T = np.linspace(205.0, 285.0, np_)
            check = cs.check
            nT = np.ascontiguousarray(np.stack([T[:-1], T[1:]]), dtype=float)
            check(cs.lib().cs_column_setup(c.handle, nnu, cs.dptr(nu), None, np_, cs.dptr(P), 9.8, 2, cs.dptr(nT.ravel(order="F").copy()),
                                           cs.dptr(np.full(2 * (np_ - 1), 0.029)), cs.dptr(T), 0, None, None, None, None, 0.0, None, None, None,
                                           0.841, 4, 1, 1))
            check(cs.lib().cs_column_set_accel(c.handle, 1))
            check(cs.lib().cs_column_run(c.handle, None))
            sig = np.zeros((np_, nnu))
            check(cs.lib().cs_column_sigma_fetch(c.handle, nnu, np_, cs.dptr(sig)))
            for k in range(np_):
                ref, f = R.accel_sigma(L, Pk, P[k])
                ok = ref > 1e-290
                assert np.all(np.abs(sig[k][ok] - ref[ok]) <= R.accel_bound(L, f) * ref[ok]), (np_, k)
    finally:
        c.close()
