"""Shape code 5 (Van Vleck-Huber Voigt, include/clearsky_hip.h) on the host side: the code in every table that maps shape names, the
Julia binding's drop-in and scalar method, the product header's prototype count left as it was, and the numpy restatement the GPU
tests build their expected values from, checked against the definition in 40-digit arithmetic.  No GPU needed."""
import inspect
import os
import re

import mpmath as mp
import numpy as np
import pytest

from conftest import HITRAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT = 25.0


def _read(*p):
    with open(os.path.join(ROOT, *p), encoding="utf-8") as f:
        return f.read()


def test_python_shape_code(cs):
    assert cs.SHAPES["voigtVVH"] == 5
    assert {k: cs.SHAPES[k] for k in ("voigt", "lorentz", "doppler", "PHCO2", "phco2", "voigtCKD")} == \
        {"voigt": 0, "lorentz": 1, "doppler": 2, "PHCO2": 3, "phco2": 3, "voigtCKD": 4}
    assert callable(cs.voigtVVH) and callable(cs.voigtVVH_)
    assert inspect.signature(cs.voigtVVH).parameters["dnu_cut"].default == 25.0


def test_header_enum():
    h = _read("include", "clearsky_hip.h")
    enum = re.search(r"enum\s*\{\s*CS_SHAPE_VOIGT\s*=\s*0[^}]*\}", h).group(0)
    assert re.search(r"CS_SHAPE_VOIGT_VVH\s*=\s*5", enum)
    # an enum value, not a prototype: the product header keeps its 48 entry points
    src = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", h, flags=re.S))
    protos = set(re.findall(r"\b(?:const\s+)?(?:int|void|char)\s*\**\s*(cs_\w+)\s*\([^;{]*?\)\s*;", src, flags=re.S))
    assert len(protos) == 48, len(protos)


def test_julia_binding():
    j = _read("julia", "ClearSkyHIP.jl")
    assert re.search(r"const SHAPES = Dict\([^)]*:voigtVVH=>5", j)
    assert re.search(r"^hipvoigtVVH!\(σ, ν, sl, T, P, Pₚ, Δνcut=25\.0\) = hipshape!\(:voigtVVH,", j, re.M)
    assert re.search(r"^function voigtVVH\(ν::Real, sl::SpectralLines, T, P, Pₚ, Δνcut=25\.0\)", j, re.M)
    assert "ClearSky.fvoigt" in j and "g.shape == :voigtVVH ? voigtVVH" in j
    assert re.search(r"^export .*hipvoigtVVH!", j, re.M)
    declared = set(re.findall(r"\b(cs_\w+)\s*\(", _read("include", "clearsky_hip.h") + _read("include", "clearsky_hip_dev.h")))
    assert set(re.findall(r"ccall\(\(:(cs_\w+)", j)) <= declared


def test_gas_objects_accept_the_shape(cs):
    nu = np.linspace(1500.0, 1600.0, 11)
    sl = cs.SpectralLines.synthetic(1, 20, 3, 1490.0, 1610.0)
    g = cs.DirectGas(sl, 0.01, nu, shape="voigtVVH")
    assert g.dnu_cut == 25.0 and cs.SHAPES[g.shape] == 5


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

def c2(cs):
    C_ = cs.constants
    return 100.0 * C_.h * C_.c / C_.k


def R(cs, x, T):
    """R(x, T) = x tanh(c2 x / 2T)"""
    return x * np.tanh(c2(cs) * x / (2.0 * T))


def restate(cs, O, sl, nu, T, P, Pp, cut=CUT, strict=True):
    """sigma_5 at the points nu, written out: S~_l = S_l / R(nul, T) (with the factor 1 - exp(-c2 nul / T) of S_l cancelled against
    tanh, so that no difference of nearly equal numbers is formed), alpha_l and gamma_l as the Voigt shape takes them, the profile
    as fvoigt with the oracle's Re w; the direct term where |nu - nul| <= cut, the mirror term where nu + nul <= cut; strict: the
    vector methods' end-point pre-filter on nul"""
    C_ = cs.constants
    nu = np.asarray(nu, float)
    keep = (sl.nu > nu[0] - cut) & (sl.nu < nu[-1] + cut) if strict else np.ones(len(sl.nu), bool)
    j = np.nonzero(keep)[0]
    nul, E, I = sl.nu[j], sl.Epp[j], sl.I[j]
    k2 = c2(cs)
    qr = np.array([O.chebyQrefQ(T, sl.cheb[i][: sl.ncheb[i]]) if sl.ncheb[i] > 0 else np.nan for i in range(len(sl.ncheb))])
    d0 = np.exp(-k2 * E / C_.Tref) * (1.0 - np.exp(-k2 * nul / C_.Tref))
    St = sl.S[j] * qr[I - 1] * np.exp(-k2 * E / T) * (1.0 + np.exp(-k2 * nul / T)) / (nul * d0)
    alpha = (nul / C_.c) * np.sqrt(2.0 * C_.R * T / sl.mu[j])
    gamma = (C_.Tref / T) ** sl.na[j] * (sl.gamma_a[j] * (P - Pp) + sl.gamma_s[j] * Pp) / C_.atm
    dd = np.sqrt(np.log(2.0)) / alpha
    A = St * np.sqrt(np.log(2.0) / np.pi) / alpha
    out = np.zeros(len(nu))
    for i, v in enumerate(nu):
        dv = v - nul
        m = ~(np.abs(dv) > cut)
        s = np.sum(A[m] * O.faddeeva(dv[m] * dd[m], gamma[m] * dd[m])) if m.any() else 0.0
        mm = ~(v + nul > cut)
        if mm.any():
            s += np.sum(A[mm] * O.faddeeva((v + nul[mm]) * dd[mm], gamma[mm] * dd[mm]))
        out[i] = R(cs, v, T) * s
    return out


def _exact(cs, O, sl, v, T, P, Pp, cut, lines):
    """the definition at 40 digits: S_l(T) as scaleintensity writes it, divided by R(nul, T); Voigt as Re w(z) = Re exp(-z^2) erfc(-iz)"""
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
        # (the normalisation at Tref as every shape takes it, in float64: for nul = 8.4e-5 its 1 - exp(.) carries 2e-10 of rounding,
        # the same in code 0 and in the reference; what is new here is the factor at T, cancelled against R(nul, T))
        k2f = c2(cs)
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
        term = mp.mpf(0)
        if abs(v - nul) <= cut:
            term += f(v - nul)
        if v + nul <= cut:
            term += f(v + nul)
        tot += S / Rm(nul) * term
    return float(Rm(v) * tot)


@pytest.fixture(scope="module")
def low_h2o(cs):
    """the golden H2O lines below 40 cm^-1 (the lowest at 8.4e-5 cm^-1)"""
    return cs.SpectralLines(os.path.join(HITRAN, "H2O.par"), numin=0.0, numax=40.0)


def test_restatement_vs_definition(cs, O, low_h2o):
    sl = low_h2o
    assert sl.nu[0] < 1e-4 and len(sl.nu) >= 13
    T, P, Pp = 250.0, 3e4, 300.0
    # nu -> 0, mirror points (nu + nul <= cut for the low lines), both sides of the mirror edge of the lowest lines, a point beyond it
    pts = np.array([1e-9, 1e-4, 8.4e-5, 0.5, 3.0, 11.7, CUT - sl.nu[3], CUT - sl.nu[3] + 1e-6, 24.0, 30.0])
    for strict in (True, False):
        r = restate(cs, O, sl, pts, T, P, Pp, strict=strict)
        assert np.all(np.isfinite(r)) and np.all(r >= 0)
        keep = (sl.nu > pts[0] - CUT) & (sl.nu < pts[-1] + CUT) if strict else np.ones(len(sl.nu), bool)
        for i, v in enumerate(pts):
            e = _exact(cs, O, sl, v, T, P, Pp, CUT, np.nonzero(keep)[0])
            assert abs(r[i] - e) <= 1e-13 * abs(e), (v, r[i], e)
    # nu = 0 exactly: zero, not NaN
    assert restate(cs, O, sl, [0.0, 1.0], T, P, Pp)[0] == 0.0


def test_wing_ratios_of_the_issue(cs):
    """R(nu)/R(nul) against the plain Voigt wing at 250 K, as the issue quotes them (x1.54 / x0.57 at nul = 100 cm^-1, +-25)"""
    T = 250.0
    for nul, hi, lo in ((100.0, 1.54, 0.57), (400.0, 1.09, 0.91), (1000.0, 1.026, 0.974)):
        assert abs(R(cs, nul + 25.0, T) / R(cs, nul, T) - hi) < 0.01 * hi
        assert abs(R(cs, nul - 25.0, T) / R(cs, nul, T) - lo) < 0.01 * lo
