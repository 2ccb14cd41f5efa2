"""Shape code 4 (pedestal-removed Voigt, include/clearsky_hip.h) on the host side: the code in every table that maps shape names, the
Julia binding's drop-in and scalar method, and the product header's prototype count left as it was.  No GPU needed."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    with open(os.path.join(ROOT, *p), encoding="utf-8") as f:
        return f.read()


def test_python_shape_code(cs):
    assert cs.SHAPES["voigtCKD"] == 4
    assert {k: cs.SHAPES[k] for k in ("voigt", "lorentz", "doppler", "PHCO2", "phco2")} == \
        {"voigt": 0, "lorentz": 1, "doppler": 2, "PHCO2": 3, "phco2": 3}
    assert callable(cs.voigtCKD) and callable(cs.voigtCKD_)
    import inspect
    assert inspect.signature(cs.voigtCKD).parameters["dnu_cut"].default == 25.0


def test_header_enum():
    h = _read("include", "clearsky_hip.h")
    enum = re.search(r"enum\s*\{\s*CS_SHAPE_VOIGT\s*=\s*0[^}]*\}", h).group(0)
    assert re.search(r"CS_SHAPE_VOIGT_CKD\s*=\s*4", enum)
    # an enum value, not a prototype: the product header keeps its 48 entry points
    src = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", h, flags=re.S))
    protos = set(re.findall(r"\b(?:const\s+)?(?:int|void|char)\s*\**\s*(cs_\w+)\s*\([^;{]*?\)\s*;", src, flags=re.S))
    assert len(protos) == 48, len(protos)


def test_julia_binding():
    j = _read("julia", "ClearSkyHIP.jl")
    assert re.search(r"const SHAPES = Dict\([^)]*:voigtCKD=>4", j)
    assert re.search(r"^hipvoigtCKD!\(σ, ν, sl, T, P, Pₚ, Δνcut=25\.0\) = hipshape!\(:voigtCKD,", j, re.M)
    assert re.search(r"^function voigtCKD\(ν::Real, sl::SpectralLines, T, P, Pₚ, Δνcut=25\.0\)", j, re.M)
    assert "ClearSky.fvoigt" in j and "g.shape == :voigtCKD ? voigtCKD" in j
    assert re.search(r"^export .*hipvoigtCKD!", j, re.M)
    # no new ccall form: every ccall names a symbol the headers declare
    declared = set(re.findall(r"\b(cs_\w+)\s*\(", _read("include", "clearsky_hip.h") + _read("include", "clearsky_hip_dev.h")))
    assert set(re.findall(r"ccall\(\(:(cs_\w+)", j)) <= declared


def test_gas_objects_accept_the_shape(cs):
    nu = np.linspace(1500.0, 1600.0, 11)
    sl = cs.SpectralLines.synthetic(1, 20, 3, 1490.0, 1610.0)
    g = cs.DirectGas(sl, 0.01, nu, shape="voigtCKD")
    assert g.dnu_cut == 25.0 and cs.SHAPES[g.shape] == 4
