"""Holds tests/tabulated_ref.py -- the 40-digit references of CIA bands, opacity tables and the accelerated absorber -- to the rest of the
project, on the CPU: against the oracle's and the host functor's double restatements on the HITRAN .cia fixtures and on every synthetic
set the GPU tests use, and against the geometry those tests are named for (bands per 64-point tile, counted from the grid and the band
ends alone)."""
import math
import os

import numpy as np
import pytest

import tabulated_ref as R
from conftest import HITRAN


def _sets():
    nu = R.grid(200)
    return {"overlap1": (R.overlap_set(1), nu), "overlap2": (R.overlap_set(2), nu), "overlap3": (R.overlap_set(3), nu),
            "overlap4": (R.overlap_set(4), nu), "overlap5": (R.overlap_set(5), nu), "bands24": (R.many_bands(24), nu),
            "ends": (R.ends_set(R.grid(193)), R.grid(193)), "singles": (R.singles_set(R.grid(130)), R.grid(130)),
            "nt2": (R.band(R.NU0 - 1, R.NU0 + 60, 9, (200.0, 300.0), 3), nu)}


def _three_ways(cs, O, data, nu, T, extrap, singles):
    Pa, P1, P2 = 7.3e4, 6.1e4, 5.9e4
    x = cs.CIATables(data, extrapolate=extrap, singles=singles)
    with np.errstate(invalid="ignore", over="ignore"):
        host = np.array([cs.cia(float(v), x, T, Pa, P1, P2) for v in nu])
        orc = O.cia_sigma(data, nu, T, Pa, P1, P2, extrap, singles)
    ref = R.cia_sigma(data, nu, T, Pa, P1, P2, extrap, singles)
    return host, orc, ref


@pytest.mark.parametrize("name", sorted(_sets()))
def test_cia_reference_vs_oracle_and_host_functor_synthetic(cs, O, name):
    """NaN positions equal, finite values to 1e-13 relative and within 1 x the derived bound (tabulated_ref.cia_bound): both are double
    restatements of <= 10 flops on |ln k| <= 120"""
    data, nu = _sets()[name]
    assert R.max_abs_lnk(data) <= 120.0
    bound = R.cia_bound(data)
    assert bound < 1e-12
    seen = 0
    for extrap, singles in ((False, False), (True, False), (False, True), (True, True)):
        for T in (150.0, 180.0, 199.0, 220.0, 251.7, 340.0, 400.0):
            host, orc, ref = _three_ways(cs, O, data, nu, T, extrap, singles)
            for other in (host, orc):
                assert np.array_equal(np.isnan(other), np.isnan(ref))
                ok = ~np.isnan(ref)
                assert np.array_equal(other[ok] == 0.0, ref[ok] == 0.0)
                nz = ok & (ref != 0.0)
                if nz.any():
                    err = float(np.max(np.abs(other[nz] - ref[nz]) / ref[nz]))
                    assert err <= 1e-13 and err <= bound, (err, bound)
                    seen += int(nz.sum())
    assert seen > 0
    if name == "singles":
        _, _, ref = _three_ways(cs, O, data, nu, 250.0, False, True)
        assert 0 < np.isnan(ref).sum() < len(nu) and np.isfinite(ref).sum() > 0


@pytest.mark.parametrize("fn", ["CO2-CO2_2018.cia", "CO2-CH4_2018.cia"])
def test_cia_reference_vs_oracle_and_host_functor_fixtures(cs, O, fn):
    """the same on the HITRAN fixtures.  1e-13 is the figure for |ln k| <= 120; the fixtures also hold k <= 0 samples, clamped to floatmin
    (ln k = -708), and a point whose cell touches one is held to the derived bound 12 U max|ln k| + 8 U of the file instead (9.5e-13)"""
    data = cs.readcia(os.path.join(HITRAN, fn))
    nu = np.concatenate([np.linspace(1.0, 3300.0, 97), [1.0, 750.0, 1000.0, 1800.0, 2510.0, 2850.0, 2850.04, 2850.819, 3249.583, 750.0000001]])
    bound = R.cia_bound(data)
    for extrap, singles, T in ((False, False, 288.0), (True, False, 150.0), (False, True, 250.0), (True, True, 900.0)):
        host, orc, ref = _three_ways(cs, O, data, nu, T, extrap, singles)
        k = R.cia_k(data, nu, T, extrap, singles)
        small = np.array([q is not None and q > 0 and R.mp.log(q) < -120 for q in k])
        for other in (host, orc):
            assert np.array_equal(np.isnan(other), np.isnan(ref))
            nz = ~np.isnan(ref) & (ref != 0.0)
            assert np.array_equal(other[~np.isnan(ref)] == 0.0, ref[~np.isnan(ref)] == 0.0)
            err = np.zeros(len(nu))
            err[nz] = np.abs(other[nz] - ref[nz]) / ref[nz]
            assert np.all(err[nz & ~small] <= 1e-13), float(err[nz & ~small].max())
            assert np.all(err[nz & small] <= bound)


def test_linear_ieee_rules_are_those_of_the_expression():
    """the inf / NaN rules written into tabulated_ref._linear_ieee against the same expression in IEEE doubles (numpy)"""
    inf = np.inf
    for ya, yb in ((-inf, -inf), (-inf, -95.0), (-95.0, -inf), (-95.0, -97.0)):
        for v in (2.0, 2.25, 3.0):
            with np.errstate(invalid="ignore"):
                d = np.exp((np.float64(v) - 2.0) * (np.float64(yb) - np.float64(ya)) / (3.0 - 2.0) + np.float64(ya))
            e = R._linear_ieee(v, 2.0, 3.0, ya, yb)
            assert (e is None) == bool(np.isnan(d)), (ya, yb, v)
            if e is not None:
                assert float(e) == pytest.approx(float(d), rel=1e-13)


def test_synthetic_sets_have_the_overlap_they_are_named_for():
    s = _sets()
    for n in (1, 2, 3, 4, 5):
        ov = R.tile_overlaps(*s["overlap%d" % n])
        assert max(ov) == n and ov[1] == n
    ov5 = R.tile_overlaps(*s["overlap5"])
    assert sum(1 for o in ov5 if o > 4) == 1                        # past CS_CIA_ACT on one tile only
    data, nu = s["bands24"]
    assert len(R._groups(data)) == 24 and max(R.tile_overlaps(data, nu)) > 4
    assert len(R._groups(R.many_bands(25))) == 25
    nbs = [len(g) for g, _, _ in R._groups(s["overlap4"][0])]
    assert min(nbs) == 2 and max(nbs) > 256 and len(set(nbs)) == 4
    # the ends set: which grid points each band holds
    data, nu = s["ends"]
    held = {round(g[0], 6): int(np.sum((g[0] <= nu) & (nu <= g[-1]))) for g, _, _ in R._groups(data)}
    counts = sorted(held.values())
    assert counts == [0, 0, 9, 16, 64, 193], counts              # between points, between tiles, 41..49, 5..20, tile 1, the whole grid
    ov = R.tile_overlaps(data, nu)
    assert ov[0] == 4 and ov[1] == 2 and len(ov) == 4            # the band between the tiles reaches neither
    assert R.tile_overlaps(*s["singles"]) == [2, 2, 1]           # a single range in the second slot of tiles 0 and 1


def test_table_reference(cs, O):
    """on a knot exp(Z_knot) exactly; against the oracle's barycentric double evaluation within the derived bound"""
    nu = R.grid(5)
    for nT, nP in ((2, 2), (2, 3), (3, 3), (3, 5), (5, 5), (8, 12), (12, 24)):
        Om = cs.AtmosphericDomain((150.0, 420.0), nT, (3.0, 2e5), nP)
        Z = R.table_values(nu, nT, nP)
        assert Z.min() >= -120.0 and Z.max() <= -40.0 and len(np.unique(Z[0])) == nT * nP
        assert not np.allclose(Z[:, : min(nT, nP), : min(nT, nP)], np.transpose(Z, (0, 2, 1))[:, : min(nT, nP), : min(nT, nP)], atol=0.5)
        i, j = nT // 2, nP - 1
        s, A = R.table_sigma(Z, Om.T, Om.P, Om.T[i], Om.P[j])
        assert np.array_equal(s, np.array([float(R.mp.exp(R.mp.mpf(float(z)))) for z in Z[:, i, j]]))
        for T, P in ((151.0, 10.0), (300.3, 1.9e5), (419.99, 3.0), (Om.T[0], 555.0), (np.nextafter(Om.T[-1], 0), Om.P[0])):
            s, A = R.table_sigma(Z, Om.T, Om.P, T, P)
            o = O.table_sigma(Z, Om.T, Om.P, T, P)
            assert np.all(np.abs(o - s) / s <= R.table_bound(nT, nP, A)), (nT, nP, T, P, np.max(np.abs(o - s) / s / R.table_bound(nT, nP, A)))


def test_accel_reference():
    Pk = np.array([10.0, 100.0, 1e4])
    L = np.array([[-100.0, -50.0], [-90.0, -60.0], [-95.0, -41.0]])
    s, f = R.accel_sigma(L, Pk, 100.0)
    assert np.array_equal(s, np.exp(L[1])) and f == 1.0
    s, f = R.accel_sigma(L, Pk, math.sqrt(1000.0))
    assert f == 1.0 and s[0] == pytest.approx(math.exp(-92.5), rel=1e-12)
    s, f = R.accel_sigma(L, Pk, 1.0)                                 # one cell below the first knot: extrapolated
    assert f == pytest.approx(2.0) and s[0] == pytest.approx(math.exp(-110.0), rel=1e-12)
    s, f = R.accel_sigma(L, Pk, 1e6)
    assert f == pytest.approx(2.0) and s[1] == pytest.approx(math.exp(-22.0), rel=1e-12)
