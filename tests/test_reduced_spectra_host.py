"""Host side of the reduced outputs of a resident column (want_M = edges / tiles): the header's names for the values of want_M, the tile
helpers, the Python switches and the Julia binding's hipspectra.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import test_julia_binding as JB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_names_the_values_of_want_M():
    src = open(JB.HEADER).read()
    vals = dict(re.findall(r"^#define (CS_M_\w+) (\d+)\s*$", src, flags=re.M))
    assert vals == {"CS_M_NONE": "0", "CS_M_PLANES": "1", "CS_M_EDGES": "2", "CS_M_TILES": "3"}
    assert len(JB.header_prototypes()) == 48          # macros only: the ABI gained no prototype
    # the resident form's comment says what cs_column_fetch writes in each mode, and what becomes of a flux destination at setup
    flat = " ".join(src.split())
    for needle in ("[2, nnu]", "[np, ntile]", "row 0 = level 0 = TOA", "DROPPED by every * cs_column_setup"):
        assert needle in flat, needle


def test_python_modes_follow_the_header(cs):
    from clearsky_jl_amd import core
    assert (core.M_NONE, core.M_PLANES, core.M_EDGES, core.M_TILES) == (0, 1, 2, 3)
    assert [core.m_mode(x) for x in (False, None, 0, True, 1, "edges", "tiles")] == [0, 0, 0, 1, 1, 2, 3]
    with pytest.raises(ValueError):
        core.m_mode("planes")


@pytest.mark.parametrize("nnu", [1, 17, 63, 64, 65, 128, 2577])
def test_tile_ranges(cs, nnu):
    r = cs.tile_ranges(nnu)
    assert len(r) == -(-nnu // 64) and r[0][0] == 0 and r[-1][1] == nnu
    assert all(b - a == 64 for a, b in r[:-1]) and 1 <= r[-1][1] - r[-1][0] <= 64
    assert all(r[q][1] == r[q + 1][0] for q in range(len(r) - 1))
    with pytest.raises(ValueError):
        cs.tile_ranges(0)


def test_band_fluxes_on_a_ragged_grid(cs):
    rng = np.random.default_rng(7)
    nnu, npl = 2577, 5
    ntile = len(cs.tile_ranges(nnu))
    Fu, Fd = rng.random((npl, ntile)), rng.random((npl, ntile))
    edges = [0, 3, 4, 40, ntile]                      # the last band is the ragged tile alone
    Bu, Bd = cs.band_fluxes(Fu, Fd, edges)
    assert Bu.shape == Bd.shape == (npl, 4)
    for F, B in ((Fu, Bu), (Fd, Bd)):
        for q, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            for i in range(npl):
                assert B[i, q] == math.fsum(F[i, a:b])
        assert np.allclose(B.sum(axis=1), F.sum(axis=1), rtol=1e-15 * ntile, atol=0)       # a full partition adds up to the total
    Bu1, _ = cs.band_fluxes(Fu, Fd, np.array([2, 5]))
    assert Bu1.shape == (npl, 1) and Bu1[0, 0] == math.fsum(Fu[0, 2:5])


@pytest.mark.parametrize("edges", [[0, 2.5, 41], [0, 42], [-1, 3], [0, 5, 5, 41], [0, 7, 3], [4], [[0, 1], [2, 3]]])
def test_band_fluxes_refuses_edges_that_are_no_tile_indices(cs, edges):
    Fu = np.ones((3, 41))
    with pytest.raises(ValueError):
        cs.band_fluxes(Fu, Fu, edges)


def test_band_fluxes_refuses_other_shapes(cs):
    with pytest.raises(ValueError):
        cs.band_fluxes(np.ones((3, 41)), np.ones((3, 40)), [0, 1])
    with pytest.raises(ValueError):
        cs.band_fluxes(np.ones(41), np.ones(41), [0, 1])


def test_fluxpack_switch(cs):
    assert cs.Discretized(4, 2, fluxpack="edges").fluxpack == "edges"
    assert "edges" in repr(cs.Discretized(4, 2, fluxpack="edges"))
    assert repr(cs.Discretized(5, 2, fluxpack="bands")) == "Discretized(nstream=5, nlobatto=2, fluxpack='bands')"
    assert repr(cs.Discretized(5, 2)) == "Discretized(nstream=5, nlobatto=2)"
    for bad in ("tiles", "planes", "", "Edges"):
        with pytest.raises(ValueError):
            cs.Discretized(4, 2, fluxpack=bad)


def test_multicontext_cannot_carry_the_mode(cs):
    """cs_fluxes_discretized_multi takes no mode: the edges fluxpack and the reduced modes of Column say so before anything reaches a device"""
    mc = object.__new__(cs.MultiContext)              # (no device behind it: the refusal must come first)
    mc.ctxs = []
    nu = np.linspace(600.0, 700.0, 130)
    P = cs.pressuregrid(10.0, 1e5, 4)
    T = np.full(4, 250.0)
    gas = cs.GrayGas(1e-27, nu)
    F = cs.FluxPack(4, 130)
    with pytest.raises(TypeError, match="cs_fluxes_discretized_multi"):
        cs.radiate_(F, cs.Discretized(4, 2, fluxpack="edges"), P, 9.8, T, 0.029, 0.0, 0.0, gas, ctx=mc)
    for mode in ("edges", "tiles"):
        with pytest.raises(TypeError, match="cs_fluxes_discretized_multi"):
            cs.Column(P, 9.8, T, 0.029, None, None, gas, want_M=mode, ctx=mc)
    with pytest.raises(ValueError):
        cs.Column(P, 9.8, T, 0.029, None, None, gas, want_M="bands", ctx=mc)


def test_julia_hipspectra_binds_the_resident_form():
    src = open(JB.JL).read()
    assert "function hipspectra(" in src and re.search(r"^export .*\n?.*hipspectra", src, flags=re.M)
    start = src.index("function hipspectra(")
    body = src[start:src.index("\n# jacobian!", start)]
    calls = JB.julia_ccalls(body)
    JB._check_calls(calls, JB.header_prototypes(), "julia/ClearSkyHIP.jl: hipspectra")
    used = [c[0] for c in calls]
    for sym in ("cs_column_setup", "cs_column_run", "cs_column_fetch"):
        assert sym in used, sym
    assert used.index("cs_column_setup") < used.index("cs_column_run") < used.index("cs_column_fetch")
    assert "mode = kind == :edges ? 2 : 3" in body and "cld(nν, 64)" in body
    # INTEGRATION.md shows the same three calls
    text = open(JB.INTEGRATION).read()
    assert "hipspectra" in text
    blocks = [b for b in re.findall(r"```julia\n(.*?)```", text, flags=re.S) if "CS_M_EDGES" in b]
    assert blocks, "INTEGRATION.md has no julia block for the reduced modes"
    icalls = [c for b in blocks for c in JB.julia_ccalls(b)]
    JB._check_calls(icalls, JB.header_prototypes(), "INTEGRATION.md: reduced spectra")
    assert {"cs_column_setup", "cs_column_run", "cs_column_fetch"} <= {c[0] for c in icalls}
