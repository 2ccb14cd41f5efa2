"""Shape code 6 (pedestal-removed Van Vleck-Huber Voigt, include/clearsky_hip.h) on the host side: the code in every table that maps
shape names, the Julia binding's drop-in and scalar method, the product header's prototype count left as it was, and the restatement
the GPU tests build their expected values from (tests/ckdvvh_ref.py), checked against one-line oracle slices and against the definition
in 40-digit arithmetic.  No GPU needed."""
import inspect
import os
import re

import mpmath as mp
import numpy as np
import pytest

import ckdvvh_ref as X
from conftest import HITRAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT = X.CUT


def _read(*p):
    with open(os.path.join(ROOT, *p), encoding="utf-8") as f:
        return f.read()


def test_python_shape_code(cs):
    assert cs.SHAPES["voigtCKDVVH"] == 6
    assert {k: cs.SHAPES[k] for k in ("voigt", "lorentz", "doppler", "PHCO2", "phco2", "voigtCKD", "voigtVVH")} == \
        {"voigt": 0, "lorentz": 1, "doppler": 2, "PHCO2": 3, "phco2": 3, "voigtCKD": 4, "voigtVVH": 5}
    assert callable(cs.voigtCKDVVH) and callable(cs.voigtCKDVVH_)
    assert inspect.signature(cs.voigtCKDVVH).parameters["dnu_cut"].default == 25.0
    assert inspect.signature(cs.voigtCKDVVH_).parameters["dnu_cut"].default == 25.0


def test_header_enum():
    h = _read("include", "clearsky_hip.h")
    enum = re.search(r"enum\s*\{\s*CS_SHAPE_VOIGT\s*=\s*0[^}]*\}", h).group(0)
    assert re.search(r"CS_SHAPE_VOIGT_CKD_VVH\s*=\s*6", enum)
    assert re.search(r"CS_SHAPE_VOIGT_CKD\s*=\s*4", enum) and re.search(r"CS_SHAPE_VOIGT_VVH\s*=\s*5", enum)
    # an enum value, not a prototype: the product header keeps its 48 entry points
    src = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", h, flags=re.S))
    protos = set(re.findall(r"\b(?:const\s+)?(?:int|void|char)\s*\**\s*(cs_\w+)\s*\([^;{]*?\)\s*;", src, flags=re.S))
    assert len(protos) == 48, len(protos)


def test_julia_binding():
    j = _read("julia", "ClearSkyHIP.jl")
    assert re.search(r"const SHAPES = Dict\([^)]*:voigtCKDVVH=>6", j)
    assert re.search(r"^hipvoigtCKDVVH!\(σ, ν, sl, T, P, Pₚ, Δνcut=25\.0\) = hipshape!\(:voigtCKDVVH,", j, re.M)
    assert re.search(r"^function voigtCKDVVH\(ν::Real, sl::SpectralLines, T, P, Pₚ, Δνcut=25\.0\)", j, re.M)
    assert "g.shape == :voigtCKDVVH ? voigtCKDVVH" in j
    assert re.search(r"^export .*hipvoigtCKDVVH!", j, re.M)
    declared = set(re.findall(r"\b(cs_\w+)\s*\(", _read("include", "clearsky_hip.h") + _read("include", "clearsky_hip_dev.h")))
    assert set(re.findall(r"ccall\(\(:(cs_\w+)", j)) <= declared


def test_gas_objects_accept_the_shape(cs):
    nu = np.linspace(1500.0, 1600.0, 11)
    sl = cs.SpectralLines.synthetic(1, 20, 3, 1490.0, 1610.0)
    g = cs.DirectGas(sl, 0.01, nu, shape="voigtCKDVVH")
    assert g.dnu_cut == 25.0 and cs.SHAPES[g.shape] == 6
    # Gas (a baked table) and opacityerror take the name through the same table; the shape reaches the library as its code
    assert "shape" in inspect.signature(cs.Gas).parameters and "shape" in inspect.signature(cs.opacityerror).parameters


@pytest.fixture(scope="module")
def low_h2o(cs):
    """the golden H2O lines below 150 cm^-1 (the lowest at 8.4e-5 cm^-1)"""
    return cs.SpectralLines(os.path.join(HITRAN, "H2O.par"), numin=0.0, numax=150.0)


def test_line_terms_vs_one_line_slices(cs, O, low_h2o):
    """S~_l f_l(x) of the restatement = the oracle's Voigt of the one-line S~-scaled slice at nul + x"""
    sl = low_h2o
    for T, P, Pp in ((220.0, 50.0, 0.02), (296.0, 101325.0, 40.53)):
        for x in (CUT, 3.0, 0.0):
            v = X.line_terms(cs, O, sl, np.full(len(sl.nu), x), T, P, Pp, np.arange(len(sl.nu)))
            ref = np.array([O.shape_bang("voigt", [sl.nu[l] + x], X.tilde(cs, sl, T, l, l + 1), T, P, Pp, 2.0 * CUT, strict_ends=False)[0]
                            for l in range(len(sl.nu))])
            assert np.max(np.abs(v - ref) / ref) < 1e-12, (T, x)


def _exact(cs, O, sl, v, T, P, Pp, cut, lines, ped=True, vvh=True):
    """the definition at 40 digits: S_l(T) as scaleintensity writes it, divided by R(nul, T); Voigt as Re w(z) = Re exp(-z^2) erfc(-iz);
    each resonance minus its own value at the cut-off.  vvh=False (code 4): no R and no mirror resonance; ped=False (code 5): no
    value at the cut-off subtracted and no clamp"""
    mp.mp.dps = 40
    C_ = cs.constants
    k2 = mp.mpf(100) * mp.mpf(C_.h) * mp.mpf(C_.c) / mp.mpf(C_.k)
    T_ = mp.mpf(T)
    Rm = lambda x: x * mp.tanh(k2 * x / (2 * T_))
    v = mp.mpf(v)
    tot = mp.mpf(0)
    for l in lines:
        nul = mp.mpf(sl.nu[l])
        i = sl.I[l]
        qr = mp.mpf(O.chebyQrefQ(T, sl.cheb[i - 1][: sl.ncheb[i - 1]]))
        E = mp.mpf(sl.Epp[l])
        # (the normalisation at Tref as every shape takes it, in float64, as in test_voigt_vvh.py)
        k2f = X.c2(cs)
        d0 = np.exp(-k2f * sl.Epp[l] / C_.Tref) * (1.0 - np.exp(-k2f * sl.nu[l] / C_.Tref))
        S = mp.mpf(sl.S[l]) * qr * (mp.exp(-k2 * E / T_) * (1 - mp.exp(-k2 * nul / T_))) / mp.mpf(d0)
        alpha = (nul / mp.mpf(C_.c)) * mp.sqrt(2 * mp.mpf(C_.R) * T_ / mp.mpf(sl.mu[l]))
        gamma = (mp.mpf(C_.Tref) / T_) ** mp.mpf(sl.na[l]) * (mp.mpf(sl.gamma_a[l]) * (mp.mpf(P) - mp.mpf(Pp)) +
                                                              mp.mpf(sl.gamma_s[l]) * mp.mpf(Pp)) / mp.mpf(C_.atm)
        dd = mp.sqrt(mp.log(2)) / alpha
        y = gamma * dd

        def f(x):
            z = mp.mpc(x * dd, y)
            return mp.sqrt(mp.log(2) / mp.pi) / alpha * mp.re(mp.exp(-z * z) * mp.erfc(-1j * z))
        pc = f(mp.mpf(cut)) if ped else mp.mpf(0)
        term = mp.mpf(0)
        if abs(v - nul) <= cut:
            term += f(v - nul) - pc
        if vvh and v + nul <= cut:
            term += f(v + nul) - pc
        rr = Rm(v) / Rm(nul) if vvh else mp.mpf(1)
        tot += S * rr * term
        if l == 0:
            t0 = abs(float(rr * S * term))
    val = float(tot)
    return (max(0.0, val) if ped else val), (t0 if 0 in lines else 0.0)


def test_restatement_vs_definition(cs, O, low_h2o):
    """ckdvvh_ref.expected (oracle Voigt of the S~ table, minus the vectorised pedestals, plus the mirror terms minus theirs, times R)
    against 40-digit arithmetic, on the golden H2O lines below 150 cm^-1: nu -> 0, the mirror region, both sides of the mirror edge of
    low lines, the direct cut-off edges, and points beyond"""
    sl = low_h2o
    assert sl.nu[0] < 1e-4 and len(sl.nu) >= 13
    T, P, Pp = 250.0, 3e4, 300.0
    lo = sl.nu[3]
    pts = np.array([1e-9, 1e-4, 8.4e-5, 0.5, 3.0, 11.7, CUT - lo - 1e-6, CUT - lo, CUT - lo + 1e-6, 24.0, 30.0, lo + CUT - 1e-3,
                    60.0, 97.3, 120.0, 149.0])
    pts = np.sort(pts)
    for strict in (True, False):
        val, scale = X.expected(cs, O, sl, pts, T, P, Pp, strict=strict)
        assert np.all(np.isfinite(val)) and np.all(val >= 0)
        keep = np.nonzero(X.included(sl, pts, CUT, strict))[0]
        for i, v in enumerate(pts):
            e, t0 = _exact(cs, O, sl, v, T, P, Pp, CUT, keep)
            # (+ the rounding of 1 - exp(-c2 nul / T) in the S~ of the line at 8.4e-5 cm^-1, eps / (c2 nul / T), on that line's term)
            assert abs(val[i] - e) <= 1e-13 * scale[i] + 5e-10 * t0 + 1e-300, (v, val[i], e, scale[i], t0)
    # nu = 0 exactly: zero, not NaN
    assert X.expected(cs, O, sl, [0.0, 1.0], T, P, Pp)[0][0] == 0.0


def test_continuous_at_the_mirror_edge(cs, O, low_h2o):
    """sigma_6 has no step at nu = cut - nul (code 5 steps there by R S~ f(cut)): one line, points 1e-9 either side"""
    sl = low_h2o
    l = int(np.argmin(np.abs(sl.nu - 10.0)))
    T, P, Pp = 296.0, 101325.0, 40.53
    e = CUT - sl.nu[l]
    keep = [l]
    a = _exact(cs, O, sl, e - 1e-9, T, P, Pp, CUT, keep)[0]
    b = _exact(cs, O, sl, e + 1e-9, T, P, Pp, CUT, keep)[0]
    step = X.R(cs, e, T) * X.line_terms(cs, O, sl, [CUT], T, P, Pp, [l])[0]
    assert abs(a - b) < 1e-6 * step


FLAGS = {4: dict(ped=True, vvh=False), 5: dict(ped=False, vvh=True), 6: dict(ped=True, vvh=True)}


def _points(sl, cut):
    """nu -> 0, points inside and beyond the cut-off, both sides of the mirror edge cut - nul and of the direct edges nul +- cut of a
    low line, all below the table's last line"""
    lo = sl.nu[3]
    p = [1e-9, 1e-4, 0.5, 3.0, 0.5 * cut, cut - lo - 1e-6, cut - lo + 1e-6, lo + cut - 1e-3, lo + cut + 1e-3, 30.0, 97.3, 149.0]
    return np.unique(np.array([x for x in p if 0.0 < x < 150.0]))


@pytest.mark.parametrize("cut", [1.0, 5.0, 25.0, 100.0])
def test_flagged_forms_at_any_cutoff(cs, O, low_h2o, cut):
    """ckdvvh_ref.expected with its flags -- code 4 (ped), code 5 (vvh), code 6 (both) -- at cut-offs 1 to 100 cm^-1: against the code-4
    restatement of test_gpu_voigt_ckd (one-line oracle slices as pedestals), the code-5 restatements of test_voigt_vvh and
    test_gpu_voigt_vvh, and the definition at 40 digits"""
    import test_gpu_voigt_ckd as CKD
    import test_gpu_voigt_vvh as GV
    import test_voigt_vvh as V
    sl = low_h2o
    T, P, Pp = 250.0, 3e4, 300.0
    x = _points(sl, cut)
    grid = np.linspace(0.5, 140.0, 400)
    # (the restatements without the line at 8.4e-5 cm^-1: test_voigt_vvh.restate cancels its 1 - exp(-c2 nul / T) exactly, line_terms
    # carries that factor's rounding, 3e-10 of the line's term -- the 40-digit check below allows for it)
    rest = CKD._slice(sl, 1, len(sl.nu))
    for strict in (True, False):
        for code, fl in FLAGS.items():
            val, scale = X.expected(cs, O, rest, grid, T, P, Pp, cut=cut, strict=strict, **fl)
            assert np.all(np.isfinite(val)) and np.all(scale >= np.abs(val)) and np.any(val > 0)
            if code == 4:
                others = [CKD.restate(O, rest, grid, T, P, Pp, cut, strict)]
            elif code == 5:
                others = [V.restate(cs, O, rest, grid, T, P, Pp, cut, strict), GV.expected(cs, O, rest, grid, T, P, Pp, cut, strict)]
                assert np.array_equal(val, scale)
            else:
                others = []
            for o in others:
                assert np.max(np.abs(o - val) / np.maximum(scale, 1e-300)) < 1e-12, (code, strict)
    # the default is code 6, bitwise
    a, b = X.expected(cs, O, sl, grid, T, P, Pp, cut=cut), X.expected(cs, O, sl, grid, T, P, Pp, cut=cut, ped=True, vvh=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the definition at 40 digits (strict: the vector methods' lines).  At 1 and 5 cm^-1 a point's value is that of one or two lines
    # near their centres, at y ~ 1e2, where the oracle's Re w is good to some 1e-11 against mpmath (7e-12 measured); from 25 cm^-1 on the
    # many lines of a window bring it to the 1e-13 of test_restatement_vs_definition
    tol = 1e-13 if cut >= 25.0 else 2e-11
    keep = np.nonzero(X.included(sl, x, cut, True))[0]
    for code, fl in FLAGS.items():
        val, scale = X.expected(cs, O, sl, x, T, P, Pp, cut=cut, **fl)
        for i, v in enumerate(x):
            e, t0 = _exact(cs, O, sl, v, T, P, Pp, cut, keep, **fl)
            assert abs(val[i] - e) <= tol * scale[i] + 5e-10 * t0 + 1e-300, (code, v, val[i], e, scale[i], t0)
