"""GPU tests of what a ClearSky.jl caller reaches through `radiate!` and of the two small members of the reference's gas surface
added in round 5:

  * radiate!(F, core, ...) (fluxes.jl:357-383) with `fluxpack="bands"` (julia/ClearSkyHIP.jl: HIPDiscretized(fluxpack=:bands)): F+, F-,
    Fnet from the device's intF! (shared.jl:125-137), tau / M+ / M- neither copied nor touched -- bitwise the band fluxes of the full
    FluxPack call, and (BASELINE configs[2] at full size) within the time heating! (radiative_convective.jl:109-144) can afford;
  * SemiGrayGas (gases.jl:366-386) through the column path against the oracle;
  * opacityerror (gases.jl:152-175) against its definition evaluated piece by piece.
"""
import math
import time

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(cs):
    c = cs.Context(0)
    yield c
    c.close()


def _small_column(cs, lines):
    import workloads as W
    nu = np.linspace(550.0, 800.0, 4001)
    P = cs.pressuregrid(1.0, 1e5, 13)
    T = W.earth_temperature(P)
    return nu, P, T, cs.DirectGas(lines("CO2"), 400e-6, nu)


def test_radiate_bands_equals_full_bitwise(cs, lines, ctx):
    nu, P, T, gas = _small_column(cs, lines)
    full = cs.FluxPack(len(P), len(nu))
    cs.radiate_(full, cs.Discretized(5, 2), P, 9.8, T, 0.029, 1e-4, 0.2, gas, ctx=ctx)
    bands = cs.FluxPack(len(P), len(nu))
    bands.tau[...] = -1.0       # sentinels: a bands call must not touch the three matrices
    bands.Mup[...] = -2.0
    bands.Mdn[...] = -3.0
    cs.radiate_(bands, cs.HIPDiscretized(5, 2, fluxpack="bands"), P, 9.8, T, 0.029, 1e-4, 0.2, gas, ctx=ctx)
    assert np.array_equal(bands.Fup, full.Fup) and np.array_equal(bands.Fdn, full.Fdn) and np.array_equal(bands.Fnet, full.Fnet)
    assert np.all(bands.tau == -1.0) and np.all(bands.Mup == -2.0) and np.all(bands.Mdn == -3.0)
    assert np.array_equal(full.Fnet, full.Fup - full.Fdn)
    # the reference's own host-side integral of what the full call returned (intF!, shared.jl:125-137) agrees with the device's
    w = cs.trapz_weights(nu)
    assert relerr(full.Fup, full.Mup @ w) < 1e-12
    # hipfluxes / hipnetfluxes (fluxes.jl:311-352 without M+, M-, tau ever leaving HBM)
    Fu, Fd = cs.hipfluxes(P, 9.8, T, 0.029, 1e-4, 0.2, gas, core=cs.Discretized(5, 2), ctx=ctx)
    assert np.array_equal(Fu, full.Fup) and np.array_equal(Fd, full.Fdn)
    assert np.array_equal(cs.hipnetfluxes(P, 9.8, T, 0.029, 1e-4, 0.2, gas, core=cs.Discretized(5, 2), ctx=ctx), full.Fnet)
    with pytest.raises(ValueError):
        cs.Discretized(5, 2, fluxpack="everything")


def test_radiate_bands_c3_time(cs):
    """BASELINE configs[2] at full size through the host-pointer entry point, as heating! would call it once per RCM step: the
    repeated bands-only call (resident column re-used, node states uploaded, 2 np doubles back) must stay within 2.5 ms -- the
    full FluxPack costs 5.2 ms + the host's serial trapz over 2 x 61 strided rows of 1e5."""
    import workloads as W
    cfg = W.config("C3")
    c = cs.Context(0)
    try:
        core = cs.HIPDiscretized(5, 2, fluxpack="bands")
        U = cs.UnifiedAbsorber(*cfg["absorbers"])
        F = cs.FluxPack(len(cfg["P"]), len(cfg["nu"]))
        args = (F, core, cfg["P"], cfg["g"], cfg["T"], cfg["mu"], cfg["fS"], cfg["fa"], U)
        cs.radiate_(*args, ctx=c)      # first call: full setup
        cs.radiate_(*args, ctx=c)
        olr = F.Fup[0]
        # the library's part of a repeated call (the Python mirror re-evaluates the closures at 1e5 wavenumbers around it, which the
        # Julia method does in compiled code): time cs_fluxes_discretized itself, marshalled as the ccall
        from clearsky_jl_amd.core import Column, _fluxes_discretized
        d = Column(cfg["P"], cfg["g"], cfg["T"], cfg["mu"], cfg["fS"], cfg["fa"], U, core=core, ctx=c, _setup=False)
        best = float("inf")
        for _ in range(8):
            t0 = time.perf_counter()
            Fu, Fd = _fluxes_discretized(d, None, None, None)
            best = min(best, (time.perf_counter() - t0) * 1e3)
        assert Fu[0] == olr
        assert 50.0 < olr < 400.0
        assert best <= 2.5, f"bands-only radiate! call took {best:.2f} ms"
    finally:
        c.close()


def test_semigray_column_vs_oracle(cs, O, lines, ctx):
    """SemiGrayGas beside a line-by-line gas: sigma below nu_cut, nothing above (gases.jl:386), every output against the oracle."""
    nu, P, T, gas = _small_column(cs, lines)
    semi = cs.SemiGrayGas(3e-26, nu, 700.0)
    assert semi(0, 250.0, 1e4) == 3e-26 and semi(len(nu) - 1, 250.0, 1e4) == 0.0
    F = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, gas, semi, core=cs.Discretized(5, 2), ctx=ctx)
    col = cs.Column(P, 9.8, T, 0.029, 0.0, 0.0, gas, semi, core=cs.Discretized(5, 2), ctx=ctx, _setup=False)
    extra = np.tile(np.where(nu <= 700.0, 3e-26, 0.0), (col.K, 1))
    r = O.fluxes_discretized(nu, P, 9.8, 2, col.Tn, col.mun, col.Tlev, [gas.sl], ["voigt"], [25.0], col.conc, sigma_extra=extra)
    assert relerr(F.tau, r["tau"]) < 1e-11
    sm = max(r["Mup"].max(), r["Mdn"].max())
    assert np.max(np.abs(F.Mup - r["Mup"])) < 1e-11 * sm and np.max(np.abs(F.Mdn - r["Mdn"])) < 1e-11 * sm
    assert np.max(np.abs(F.Fup - r["Fup"])) < 1e-11 * r["Fup"].max() and np.max(np.abs(F.Fdn - r["Fdn"])) < 1e-11 * r["Fup"].max()
    # the cut is felt: without the semi-gray member the optical depth below 700 cm^-1 is smaller, above it the same
    F0 = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, gas, core=cs.Discretized(5, 2), ctx=ctx)
    lo, hi = nu <= 700.0, nu > 700.0
    assert np.all(F.tau[:, lo] >= F0.tau[:, lo]) and np.any(F.tau[:, lo] > F0.tau[:, lo]) and np.array_equal(F.tau[:, hi], F0.tau[:, hi])
    # alone it cannot carry a column (a UnifiedAbsorber needs wavenumbers: it has them) -- and does
    F1 = cs.radiate(P, 9.8, T, 0.029, 0.0, 0.0, semi, core=cs.Discretized(5, 2), ctx=ctx)
    r1 = O.fluxes_discretized(nu, P, 9.8, 2, col.Tn, col.mun, col.Tlev, [], [], [], np.zeros((0, col.K)), sigma_extra=extra)
    assert relerr(F1.tau, r1["tau"]) < 1e-12 and relerr(F1.Fup, r1["Fup"]) < 1e-12


def test_opacityerror_vs_definition(cs, lines, ctx):
    """opacityerror(Pi, Omega, sl, nu, C, shape, N) (gases.jl:152-175): interpolated minus exact on the N x N grid of the domain."""
    nu = np.linspace(660.0, 680.0, 257)
    Om = cs.AtmosphericDomain((180.0, 320.0), 8, (10.0, 1e5), 12)
    fC = lambda T, P: 400e-6
    g = cs.Gas(lines("CO2"), fC, nu, Om, ctx=ctx)
    i, N = 100, 7
    T, P, aerr, rerr = cs.opacityerror(g, i, N)
    assert T.shape == (N,) and P.shape == (N,) and aerr.shape == (N, N) and rerr.shape == (N, N)
    assert T[0] == Om.Tmin and abs(T[-1] - Om.Tmax) < 1e-12 and abs(P[0] - Om.Pmin) < 1e-9 and abs(P[-1] / Om.Pmax - 1) < 1e-12
    for a in (0, 3, 6):
        for b in (0, 2, 6):
            ex = cs.voigt(float(nu[i]), lines("CO2"), T[a], P[b], fC(T[a], P[b]) * P[b], ctx=ctx)     # the scalar-nu method
            op = g.rawsigma(T[a], P[b], i)
            assert abs(aerr[a, b] - (op - ex)) <= 1e-13 * abs(ex) and abs(rerr[a, b] - (op - ex) / ex) <= 1e-10
    assert np.max(np.abs(rerr)) < 0.1       # "about 1 %" with a production grid (gases.jl:7); this one is coarse


def test_opacityerror_of_a_reconcentrated_gas(cs, lines, ctx):
    """opacityerror's exact values take the concentration the table was baked with (its self-broadening), not the view's new one: for a
    reconcentrate()d gas it reports the same interpolation error as for the gas it came from"""
    nu = np.linspace(660.0, 680.0, 65)
    Om = cs.AtmosphericDomain((180.0, 320.0), 5, (10.0, 1e5), 6)
    g = cs.Gas(lines("CO2"), 0.3, nu, Om, ctx=ctx)
    g2 = g.reconcentrate(0.01)
    a, b = cs.opacityerror(g, 30, 5), cs.opacityerror(g2, 30, 5)
    assert g2.fC(250.0, 1e4) == 0.01 and g2.fC_bake(250.0, 1e4) == 0.3
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    T, P = a[0], a[1]
    ex = cs.voigt(float(nu[30]), lines("CO2"), T[2], P[3], 0.3 * P[3], ctx=ctx)
    assert abs(b[2][2, 3] - (g2.rawsigma(T[2], P[3], 30) - ex)) <= 1e-13 * abs(ex)
    other = cs.voigt(float(nu[30]), lines("CO2"), T[2], P[3], 0.01 * P[3], ctx=ctx)
    assert abs(other - ex) > 1e-3 * abs(ex)                             # (the self-broadening matters at this point)


def test_band_fluxes_written_into_caller_memory(cs, lines, ctx):
    """cs_column_set_flux_dst: the flux kernel's last blocks (or k_freduce) write [Fup; Fdn] straight into caller-owned device memory --
    the tensor a collective reduces in place -- bitwise what the column's own buffer gets, for every later run until the column is set up
    again; fetch / flux_to follow the destination.  The "caller-owned" memory here is the band-flux buffer of a column on ANOTHER context
    (2 np doubles the library itself allocated: no second HIP runtime in the process), read back through that column's fetch."""
    nu, P, T, gas = _small_column(cs, lines)
    col = cs.Column(P, 9.8, T, 0.029, 1e-4, 0.2, gas, core=cs.Discretized(5, 2), ctx=ctx)
    col.run()
    F0 = np.concatenate(col.fetch())
    other_ctx = cs.Context(0)
    try:
        col2 = cs.Column(P, 9.8, T + 5.0, 0.029, 1e-4, 0.2, gas, core=cs.Discretized(5, 2), ctx=other_ctx)
        col2.run()
        F2 = np.concatenate(col2.fetch())
        assert not np.array_equal(F2, F0)
        dst = col2.flux_ptr()                       # device memory this column does not own
        col.set_flux_dst(dst)
        col.run()
        col.sync()
        assert np.array_equal(np.concatenate(col2.fetch()), F0)           # ... now holds this column's band fluxes
        assert np.array_equal(np.concatenate(col.fetch()), F0) and col.flux_ptr() == dst
        # new temperatures on the resident column: the destination holds
        col.update(T + 2.0)
        col.run()
        col.sync()
        F1 = np.concatenate(col2.fetch())
        assert not np.array_equal(F1, F0) and np.array_equal(np.concatenate(col.fetch()), F1)
        # back to the column's own buffer: the foreign one is left alone, flux_to copies on request
        col.set_flux_dst(0)
        col2.run()
        col2.sync()
        assert np.array_equal(np.concatenate(col2.fetch()), F2)
        col.run()
        col.sync()
        assert np.array_equal(np.concatenate(col2.fetch()), F2) and np.array_equal(np.concatenate(col.fetch()), F1)
        col.flux_to(dst)
        col.sync()
        assert np.array_equal(np.concatenate(col2.fetch()), F1)
    finally:
        col.set_flux_dst(0)
        other_ctx.close()
