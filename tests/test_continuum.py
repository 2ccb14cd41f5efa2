"""CS_CIA_RADIATION and Continuum on the host side: the header's names, the flag Column._set_cia emits, the unit mapping of Continuum
against the MT_CKD formula in 40-digit mpmath, the host functor's R, the Julia glue, and the premise of the device cases (a good share
of the reference's layer optical depths above the 1e-6 floor).  No GPU needed."""
import os
import re

import mpmath as mp
import numpy as np
import pytest

import continuum_ref as CR
import tabulated_ref as R
from conftest import ROOT

mp.mp.dps = 40


def _read(*p):
    with open(os.path.join(ROOT, *p), encoding="utf-8") as f:
        return f.read()


def test_header_names():
    h = _read("include", "clearsky_hip.h")
    for name, v in (("CS_CIA_EXTRAPOLATE", 1), ("CS_CIA_SINGLES", 2), ("CS_CIA_RADIATION", 4)):
        assert re.search(rf"#define\s+{name}\s+{v}\b", h), name
    assert "R(nu, T) = nu tanh(c2 nu / 2T)" in h and "ln(C / n_ref)" in h
    # three names, no prototype: the product header keeps its 48 entry points (the regex of tests/test_voigt_ckd.py)
    src = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", h, flags=re.S))
    protos = set(re.findall(r"\b(?:const\s+)?(?:int|void|char)\s*\**\s*(cs_\w+)\s*\([^;{]*?\)\s*;", src, flags=re.S))
    assert len(protos) == 48, len(protos)
    from clearsky_jl_amd import _lib
    assert (_lib.CS_CIA_EXTRAPOLATE, _lib.CS_CIA_SINGLES, _lib.CS_CIA_RADIATION) == (1, 2, 4)
    assert len(_lib.SIGNATURES) == 62      # (+ cs_phco2_plan_ctx, cs_phco2_wide_regions: test hooks of clearsky_hip_dev.h)


def _h2o(cs, nu, x=0.02):
    return cs.DirectGas(cs.SpectralLines.synthetic(1, 20, 3, 5000.0, 5100.0), x, nu)


def _coeff(nu, T):
    return 3e-23 * np.exp(-np.asarray(nu) / 300.0) * (296.0 / T) ** 3


def test_set_cia_flags(cs, monkeypatch):
    """Column._set_cia: bit 2 for a Continuum and for CIATables(radiation=True), 0 .. 3 otherwise"""
    from clearsky_jl_amd import core
    nu = np.linspace(10.0, 60.0, 11)
    g = _h2o(cs, nu)
    ns = np.linspace(5.0, 70.0, 9)
    two = cs.Continuum([dict(nu=ns, T=t, C=_coeff(ns, t)) for t in (250.0, 300.0)], g, "self")
    one = cs.Continuum({296.0: _coeff(ns, 296.0)}, g, "foreign", nu=ns)
    band = R.band(5.0, 70.0, 7, R.TS, 1, "H2O-H2O")
    tabs = [cs.CIATables(band, extrapolate=e, singles=s, radiation=r) for e, s, r in
            ((False, False, False), (True, False, False), (False, True, False), (True, True, False), (False, False, True), (True, True, True))]
    seen = {}

    class FakeLib:
        def cs_column_set_cia(self, h, n, slots, flags, p1, p2):
            seen["flags"] = [flags[i] for i in range(n)]
            return 0

    class FakeCtx:
        handle = None

        def cia_slot(self, x):
            return 0
    monkeypatch.setattr(core, "lib", lambda: FakeLib())
    for members, want in (([two], [4]), ([one], [6]), (tabs[:4], [0, 1, 2, 3]), (tabs[4:], [4, 7]), ([tabs[1], two, tabs[2]], [1, 4, 2])):
        col = object.__new__(cs.Column)
        col.U, col.ctx = cs.UnifiedAbsorber(g, *members), FakeCtx()
        col.cia_P1 = col.cia_P2 = np.zeros((len(members), 3), order="F")
        col._set_cia()
        assert seen["flags"] == want, (seen["flags"], want)
    assert two.x.radiation and not two.x.extrapolate and not two.x.singles
    assert one.x.radiation and not one.x.extrapolate and one.x.singles      # one temperature: a single range, evaluated at every T


def test_batch_rows_are_the_states_own_arrays(cs, monkeypatch):
    """Row b of what run_batch hands to cs_column_batch -- [B][n K], member t of node k at t + n k -- is what _state leaves for profile b
    in conc, conc_tab, cia_P1 and cia_P2 (Column._node_inputs forms both), with two members of every kind whose values depend on T"""
    import ctypes as C
    from clearsky_jl_amd import core
    nu = np.linspace(10.0, 60.0, 11)
    seen = {}

    real = core.lib()

    class FakeLib:
        def cs_column_batch(self, h, B, Tn, mun, Tlev, conc, ctab, P1, P2, Fup, Fdn):
            for name, p in (("conc", conc), ("conc_tab", ctab), ("cia_P1", P1), ("cia_P2", P2)):
                seen[name] = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(B, 2 * 9)).copy()
            return 0

        def __getattr__(self, name):      # (the host-only helpers: cs_lobattonodes)
            assert name == "cs_lobattonodes", name
            return getattr(real, name)

    class FakeCtx:
        handle = None

        def slots_of(self, tables, shifts=None):
            return [0] * len(tables)
    ctx = FakeCtx()
    sl = {f: cs.SpectralLines.synthetic(m, 20, 3, 5000.0, 5100.0) for f, m in (("H2O", 1), ("CO2", 2))}
    direct = [cs.DirectGas(sl["H2O"], lambda T, P: 0.02 * (T / 250.0), nu), cs.DirectGas(sl["CO2"], lambda T, P: 0.3 + 1e-4 * T, nu)]
    baked = []
    for f in (lambda T, P: 0.1 + 2e-4 * T, lambda T, P: 0.5 * (200.0 / T)):      # two baked gases without a bake: what a Column reads of them
        g = object.__new__(cs.Gas)
        g.ctx, g.fC, g.nu, g.formula, g.Omega = ctx, f, nu, "N2", cs.AtmosphericDomain((100.0, 500.0), 2, (1.0, 2e5), 2)
        baked.append(g)
    pairs = [cs.CIATables(R.band(5.0, 70.0, 7, R.TS, 1, sym)) for sym in ("H2O-CO2", "CO2-H2O")]
    P = cs.pressuregrid(100.0, 1e5, 5)
    Ts = [np.linspace(200.0, 300.0, 5), np.linspace(260.0, 240.0, 5), np.full(5, 280.0)]
    monkeypatch.setattr(core, "lib", lambda: FakeLib())
    col = cs.Column(P, 9.8, Ts[0], 0.029, 0.0, 0.0, *direct, *baked, *pairs, core=cs.Discretized(4, 3), ctx=ctx, _setup=False, _warn=False)
    assert col.K == 9 and (len(col.gases), len(col.baked), len(col.U.cia)) == (2, 2, 2)
    ctx._resident = col
    col.run_batch(Ts)
    for b, T in enumerate(Ts):
        col._state(core.formprofile(P, T), col._fmu)
        for name in ("conc", "conc_tab", "cia_P1", "cia_P2"):
            a = getattr(col, name)
            assert a.shape == (2, 9) and a.flags.f_contiguous and not np.array_equal(a[0], a[1]), name
            assert np.array_equal(seen[name][b], a.ravel(order="F")), (name, b)
    assert not np.array_equal(seen["cia_P1"][0], seen["cia_P1"][1]) and not np.array_equal(seen["cia_P1"], seen["cia_P2"])


@pytest.mark.parametrize("kind", ["self", "foreign"])
def test_unit_mapping(cs, kind):
    """Continuum(nu, T, P) against x1 R C n2 / n_ref at table samples and temperatures (where ln C is a knot value).  The CIA functor
    reaches x1 n2 as Lo^2 rho1 rho2 / rhoa, which equals it when Lo = 1e-6 atm / (k T0); the reference's constants (Lo^2 of nine digits
    beside the CODATA-2014 k) miss that by the factor `q` formed below, some 4e-8 from 1 -- the size of the statement
    "Continuum is the MT_CKD formula".  With q taken out, what is left is double rounding: a dozen operations and one exponential of a
    knot value, 1e-13 at the most."""
    x, P_ref, T_ref = 0.013, 101325.0, 296.0
    ns = np.linspace(5.0, 2000.0, 12)
    Ts = (220.0, 260.0, 296.0, 320.0)
    nu = np.linspace(10.0, 60.0, 5)
    g = _h2o(cs, nu, x)
    c = cs.Continuum([dict(nu=ns, T=t, C=_coeff(ns, t)) for t in Ts], g, kind, P_ref=P_ref, T_ref=T_ref)
    kB = mp.mpf(cs.constants.k)
    q = mp.mpf(cs.constants.Lo2) / (mp.mpf("1e-6") * mp.mpf(cs.constants.atm) / (kB * mp.mpf(cs.constants.T0))) ** 2
    assert abs(q - 1) < 1e-7
    worst = 0.0
    for v in ns[[0, 3, 7, 11]]:
        for T in Ts:
            for P in (300.0, 1e5):
                x2 = mp.mpf(x) if kind == "self" else 1 - mp.mpf(x)
                n2 = mp.mpf("1e-6") * x2 * mp.mpf(P) / (kB * mp.mpf(T))
                n_ref = mp.mpf("1e-6") * mp.mpf(P_ref) / (kB * mp.mpf(T_ref))
                want = mp.mpf(x) * CR.radiation([v], T)[0] * mp.mpf(float(_coeff(v, T))) * n2 / n_ref
                worst = max(worst, float(abs(mp.mpf(c(float(v), T, P)) - q * want) / want))
    print(f"  {kind}: largest relative difference {worst:.2e} (the constants: q - 1 = {float(q - 1):.2e})")
    assert worst <= 1e-13
    assert c.n_ref == pytest.approx(2.4794e19, rel=1e-4) and c.x.name == ("H2O-H2O" if kind == "self" else "H2O-air")


def test_continuum_refuses_what_it_cannot_hold(cs):
    nu = np.linspace(10.0, 60.0, 5)
    g = _h2o(cs, nu)
    ns = np.linspace(5.0, 70.0, 9)
    c = cs.Continuum([dict(nu=ns, T=t, C=_coeff(ns, t)) for t in (250.0, 300.0)], g)
    for T in (249.9, 300.1):
        with pytest.raises(ValueError, match="outside the table's range"):
            c(20.0, T, 1e5)
    c.check_temperatures([250.0, 275.0, 300.0])
    cs.Continuum({296.0: _coeff(ns, 296.0)}, g, nu=ns)(20.0, 150.0, 1e5)          # one temperature: every T
    with pytest.raises(ValueError):
        cs.Continuum({296.0: _coeff(ns, 296.0)}, g, "both", nu=ns)
    with pytest.raises(ValueError):
        cs.Continuum({296.0: 0.0 * ns}, g, nu=ns)
    with pytest.raises(ValueError):
        cs.Continuum({296.0: _coeff(ns, 296.0)}, g)
    with pytest.raises(AssertionError):
        cs.UnifiedAbsorber(_h2o(cs, nu), c)                                       # its gas is not a member
    U = cs.UnifiedAbsorber(g, c)
    assert U.cia == (c,) and U.fun == () and c.g1 is g and c.g2 is g


def test_host_functor_applies_R(cs):
    """CIATables(radiation=True)(nu, T) = R(nu, T) x the unflagged tables' k, down to wavenumbers where tanh is its argument"""
    data = R.band(1e-3, 90.0, 40, R.TS, 2) + R.single(20.0, 60.0, 9, 250.0, 3)
    plain, rad = cs.CIATables(data, singles=True), cs.CIATables(data, singles=True, radiation=True)
    for v in (1e-3, 0.5, 7.0, 33.3, 90.0):
        for T in (180.0, 251.0, 340.0):
            want = mp.mpf(plain(v, T)) * CR.radiation([v], T)[0]
            assert abs(mp.mpf(rad(v, T)) - want) <= 6 * R.U * want, (v, T)
            assert cs.radiation_term(v, T) == pytest.approx(float(CR.radiation([v], T)[0]), rel=4 * R.U)
    assert rad(95.0, 250.0) == 0.0 and cs.radiation_term(0.0, 250.0) == 0.0
    assert cs.cia(7.0, rad, 251.0, 1e5, 2e4, 3e4) == cs.cia(rad(7.0, 251.0), 251.0, 1e5, 2e4, 3e4)


def test_julia_binding():
    j = _read("julia", "ClearSkyHIP.jl")
    assert re.search(r"const CS_CIA_EXTRAPOLATE, CS_CIA_SINGLES, CS_CIA_RADIATION = Cint\(1\), Cint\(2\), Cint\(4\)", j)
    assert re.search(r"struct HIPCIA\{T,U\}.*?radiation::Bool.*?\nend", j, re.S)
    assert re.search(r"^struct Continuum\{G\}", j, re.M) and re.search(r"^function Continuum\(data::Vector, gas; kind::Symbol=:self, P_ref=101325\.0, T_ref=296\.0\)", j, re.M)
    assert re.search(r"^radiationterm\(ν, T\) = ν\*tanh\(C₂\*ν/\(2\.0\*T\)\)", j, re.M)
    assert "χ.radiation) ? CS_CIA_RADIATION" in j and "concentration(p::ForeignPartner, T, P) = 1.0 - concentration(p.gas, T, P)" in j
    assert re.search(r"const HIPInput = Union\{AbstractGas, CIATables, Continuum, Function\}", j)
    assert re.search(r"^export .*\bContinuum\b", j, re.M)
    declared = set(re.findall(r"\b(cs_\w+)\s*\(", _read("include", "clearsky_hip.h") + _read("include", "clearsky_hip_dev.h")))
    assert set(re.findall(r"ccall\(\(:(cs_\w+)", j)) <= declared


@pytest.mark.parametrize("which,nnu,np_,nlob,seed,T", [("high", 320, 9, 3, 0, None), ("low", 192, 6, 2, 0, None), ("low", 257, 7, 3, 0, None),
                                                        ("low", 200, 6, 3, 1, "far"), ("low", 200, 7, 3, 1, None), ("low", 200, 7, 3, 1, "far"),
                                                        ("low", 200, 7, 3, 1, "ramp")])
def test_premise_of_the_device_cases(cs, O, lines, which, nnu, np_, nlob, seed, T):
    """the columns of tests/test_gpu_continuum.py's flux, update and batch cases, reference alone: at least 10 % of the layer optical
    depths lie above the 1e-6 floor (below it both sides agree trivially)"""
    nu = CR.grid(which, nnu)
    data = CR.bands_for(which, nu, seed=seed, symbol="CO2-CO2" if which == "high" else "H2O-H2O")
    T = {None: CR.profile(np_), "far": CR.profile(np_, 250.0, 338.0)[::-1].copy(), "ramp": np.full(np_, 231.0) + 3.0 * np.arange(np_)}[T]
    P = cs.pressuregrid(50.0, 1e5, np_)
    st = CR.states(cs, P, T, nlob)
    sig = CR.plane([(data, 0.9, 0.9)], nu, st)
    ref = CR.reference(O, cs, lines("CO2") if which == "high" else CR.low_lines(cs), nu, P, T, nlob, sig)
    f = float((ref["tau"] > 1e-6).mean())
    print(f"  {which} nnu {nnu} np {np_}: layer optical depths above the floor: {f:.2f}")
    assert f >= 0.1, f
    assert 4.0 * CR.bound(data, nlob) < 1e-12
