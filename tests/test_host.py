"""CPU tests of the host logic and the C-ABI surface (no compute calls: there is no GPU here)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import HITRAN, ROOT


def test_library_exports_every_declared_symbol(cs):
    """The shared library loads and exports every cs_* function include/clearsky_hip.h (product) and include/clearsky_hip_dev.h
    (measurement / tuning / test hooks) declare."""
    hdr = open(os.path.join(ROOT, "include", "clearsky_hip.h")).read() + open(os.path.join(ROOT, "include", "clearsky_hip_dev.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", hdr))
    assert len(declared) >= 20
    assert os.path.exists(cs.LIB_PATH), "libclearsky_hip.so must be built in-tree by __graft_entry__.build()"
    L = ctypes.CDLL(cs.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in the header but not exported"
    assert declared == set(cs.SIGNATURES), declared ^ set(cs.SIGNATURES)
    assert cs.lib().cs_version() >= 100


def test_work_layout_table_matches_the_header(cs):
    """The package's copy of cs_column_work's layout -- WORK_COUNT, DISPATCH_FLAGS -- against the enums of include/clearsky_hip_dev.h,
    whose CS_WORK_* values are the positions 0 .. CS_WORK_COUNT - 1 without a gap where Column.work() reads single values."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clearsky_hip_dev.h")).read(), flags=re.S)
    enum = {n: int(v) for n, v in re.findall(r"\b(CS_(?:WORK|DF)_[A-Z0-9_]+)\s*=\s*(\d+)", hdr)}
    assert enum["CS_WORK_COUNT"] == cs.WORK_COUNT == 41
    assert {n[len("CS_DF_"):]: v for n, v in enum.items() if n.startswith("CS_DF_")} == cs.DISPATCH_FLAGS
    work = sorted(v for n, v in enum.items() if n.startswith("CS_WORK_") and n != "CS_WORK_COUNT")
    assert work == [q for q in range(cs.WORK_COUNT) if q not in (28, 29, 30)], work     # (CS_WORK_FLUX_SCAN_NS names the first of four)


def test_tuning_key_table_matches_the_header(cs):
    """The package's name table of the cs_set_tuning keys against the CS_TUNE_* enum of include/clearsky_hip_dev.h: keys 0 .. 23 with only
    20 missing, and the named bits of keys 15 and 16 at the values callers have always passed as integers."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clearsky_hip_dev.h")).read(), flags=re.S)
    enum = {n: int(v) for n, v in re.findall(r"\b(CS_T(?:UNE|15|16)_[A-Z0-9_]+)\s*=\s*(\d+)", hdr)}
    keys = {n[len("CS_TUNE_"):]: v for n, v in enum.items() if n.startswith("CS_TUNE_")}
    assert keys == cs.TUNING
    assert sorted(keys.values()) == [k for k in range(24) if k != 20]
    assert {n[len("CS_T15_"):]: v for n, v in enum.items() if n.startswith("CS_T15_")} == dict(
        FORM_MASK=3, FREDUCE=4, CHUNK4=8, TABLES_ONE_THREAD=16, MULTI_RECUT=32, SCAN_STAMPS=128, NO_CASCADE_ASIDE=256, SCAN_MID=1024,
        SCAN_RECOMPUTE=2048)
    assert {n[len("CS_T16_"):]: v for n, v in enum.items() if n.startswith("CS_T16_")} == dict(PRIO_MASK=3, NEAR_TWO_LAUNCHES=4)


def test_no_oracle_in_product():
    """The shipped path must not import, link or call anything under oracle/."""
    pkg = os.path.join(ROOT, "clearsky.jl_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "oracle" not in txt.lower().replace("# oracle", ""), f"{f} mentions the oracle"


def test_product_imports_and_links_without_the_oracle():
    """Stronger than the text check: (i) the package imports, loads the HIP library and resolves every ABI symbol in a fresh
    interpreter in which `oracle` cannot be imported at all; (ii) the shared library's dynamic dependencies name no oracle object;
    (iii) with the HIP library absent the product raises instead of falling back to anything."""
    import subprocess
    import sys
    code = (
        "import sys, types\n"
        "class _Block:\n"
        "    def find_spec(self, name, path=None, target=None):\n"
        "        if name == 'oracle' or name.startswith('oracle.'):\n"
        "            raise ImportError('oracle is test infrastructure: blocked')\n"
        "sys.meta_path.insert(0, _Block())\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "import clearsky_jl_amd as cs\n"
        "L = cs.lib()\n"
        "assert all(hasattr(L, n) for n in cs.SIGNATURES)\n"
        "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)\n"
        "print('ok', len(cs.SIGNATURES))\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stderr[-1500:]
    import clearsky_jl_amd as cs
    dyn = subprocess.run(["readelf", "-d", cs.LIB_PATH], capture_output=True, text=True).stdout
    assert "NEEDED" in dyn and "oracle" not in dyn.lower()
    # a missing library raises (no fallback path); the loader takes no environment override -- the in-tree library is the one that runs
    code2 = (f"import sys, os\nsys.path.insert(0, {ROOT!r})\nos.environ['CLEARSKY_HIP_LIB'] = '/tmp/some_other_build.so'\n"
             "import clearsky_jl_amd as cs\nimport clearsky_jl_amd._lib as L\n"
             "assert L.LIB_PATH.endswith('clearsky.jl_amd/csrc/libclearsky_hip.so')\n"
             "assert cs.lib().cs_build_id().decode() == L.source_id(), 'library built from other sources: rebuild'\n"
             "L._lib = None\nL.LIB_PATH = '/nonexistent/libclearsky_hip.so'\n"
             "try:\n    L.lib()\nexcept cs.ClearSkyHIPError as e:\n    print('raised', e.code)\n")
    out2 = subprocess.run([sys.executable, "-c", code2], capture_output=True, text=True, timeout=300)
    assert out2.stdout.startswith("raised -100"), out2.stdout + out2.stderr[-800:]


def test_molparam_structure(cs):
    """Mirror of the reference's only active test, test/test_molparam.jl:1-18."""
    for M, mp in cs.MOLPARAM.items():
        assert mp.M == M
        if len(mp.I) > 1:
            assert np.all(mp.maxrelerr[mp.hascheb] <= 0.01)
            for j in range(len(mp.I)):
                assert mp.ncheb[j] == len(mp.cheb[j])
                assert not np.any(np.isnan(mp.cheb[j]))
            assert mp.A.sum() <= 1.001
    assert cs.TMIN == 25.0 and cs.TMAX == 1000.0
    assert not cs.MOLPARAM[34].hascheb[0] and not cs.MOLPARAM[42].hascheb[0]   # O, CF4: no fit (quirk 5)


@pytest.mark.parametrize("name,count,niso", [("CO2", 5599, 12), ("H2O", 3058, 7), ("CH4", 4504, 4)])
def test_readpar_fixtures(cs, name, count, niso):
    sl = cs.SpectralLines(os.path.join(HITRAN, name + ".par"))
    assert sl.N == count == len(sl.nu)
    assert np.all(np.diff(sl.nu) >= 0)
    assert set(np.unique(sl.I)) <= set(range(1, niso + 1))
    mp = cs.MOLPARAM[sl.M]
    assert np.array_equal(sl.mu, mp.mu[sl.I - 1]) and np.array_equal(sl.A, mp.A[sl.I - 1])
    assert sl.cheb.shape == (niso, 16)


def test_readpar_filters(cs):
    f = os.path.join(HITRAN, "CO2.par")
    p = cs.readpar(f, numin=600, numax=700)
    assert p["nu"].min() >= 600 and p["nu"].max() <= 700
    p2 = cs.readpar(f, I=[1])
    assert set(p2["I"]) == {"1"}
    p3 = cs.readpar(f, maxlines=100)
    assert len(p3["nu"]) == 100 and np.all(np.diff(p3["nu"]) >= 0)
    full = cs.readpar(f)
    assert np.sort(p3["S"])[0] >= np.sort(full["S"])[-100]
    with pytest.raises(AssertionError):
        cs.readpar(f, numin=1e9)
    with pytest.raises(AssertionError):
        cs.readpar("foo.txt")


@pytest.mark.parametrize("name", ["CO2", "H2O", "CH4"])
def test_native_par_parser_matches_python(cs, name):
    """cs_par_parse (mmap + threads) against the pure-Python restatement of readpar's parsing loop (par.jl:127-152)."""
    f = os.path.join(HITRAN, name + ".par")
    a, b = cs.readpar(f, native=True), cs.readpar(f, native=False)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    n = ctypes.c_int64()
    assert cs.lib().cs_par_count(f.encode(), ctypes.byref(n)) == 0 and n.value == len(a["nu"])
    assert cs.lib().cs_par_count(b"/nonexistent.par", ctypes.byref(n)) != 0


def test_first_line_fields(cs):
    p = cs.readpar(os.path.join(HITRAN, "CO2.par"))
    j = int(np.argmin(np.abs(p["nu"] - 0.757206)))
    assert p["M"][j] == 2 and p["I"][j] == "4"
    assert p["S"][j] == 1.751e-34 and p["gamma_a"][j] == 0.0927 and p["gamma_s"][j] == 0.125
    assert p["Epp"][j] == 0.0 and p["na"][j] == 0.78


def test_grids_and_quadrature_anchors(cs):
    assert np.allclose(cs.pressuregrid(1.0, 1e5, 5), [1, 5.39800207, 316.227766, 18525.3727, 1e5], rtol=1e-8)
    m, W = cs.streamnodes(5)        # SURVEY.md 4 anchors
    assert np.allclose(m, [1.00272098, 1.06949766, 1.41421356, 2.82008548, 13.58335526], rtol=1e-8)
    assert np.allclose(W, [0.08584143, 0.78311645, 1.40367707, 0.78311645, 0.08584143], rtol=1e-7)
    m2, W2 = cs.streamnodes(2)
    assert np.allclose(m2, [1.05774, 3.06856], rtol=1e-5) and np.allclose(W2, [1.52039, 1.52039], rtol=1e-5)
    x, w = cs.lobattonodes(4)
    assert np.allclose(x, [0, 0.5 - 0.5 / math.sqrt(5), 0.5 + 0.5 / math.sqrt(5), 1], atol=1e-15)
    assert np.allclose(w, [1 / 12, 5 / 12, 5 / 12, 1 / 12], atol=1e-15)
    assert cs.planck(667.0, 288.0) == pytest.approx(0.13090535521240354, rel=1e-14)
    assert cs.dtaudP(1e-20, 9.8, 0.029) == pytest.approx(2.1189798592540465, rel=1e-14)
    with pytest.raises(cs.ClearSkyHIPError):
        cs.streamnodes(99)


def test_host_quadrature_matches_golden(cs, golden):
    q = golden("quadrature")
    for n in (1, 2, 3, 5, 8, 16):
        m, W = cs.streamnodes(n)
        assert np.max(np.abs(m / q[f"m{n}"] - 1)) < 1e-13 and np.max(np.abs(W / q[f"W{n}"] - 1)) < 1e-13
    for n in (2, 3, 4, 5):
        x, w = cs.lobattonodes(n)
        assert np.max(np.abs(x - q[f"lx{n}"])) < 1e-15 and np.max(np.abs(w - q[f"lw{n}"])) < 1e-15


def test_profiles_and_lobatto_evaluations(cs):
    P = cs.pressuregrid(1.0, 1e5, 11)
    T = np.linspace(200, 288, 11)
    f = cs.AtmosphericProfile(P, T)
    assert f(P[3]) == pytest.approx(T[3], rel=1e-14)
    mid = math.exp(0.5 * (math.log(P[3]) + math.log(P[4])))
    assert f(mid) == pytest.approx(0.5 * (T[3] + T[4]), rel=1e-13)
    assert f(2e5) > T[-1]          # NoBoundaries: linear extrapolation
    Tn, mun = cs.lobattoevaluations(P, f, lambda T_, P_: 0.029, 3)
    assert Tn.shape == (3, 10) and np.all(mun == 0.029)
    assert Tn[0, 2] == pytest.approx(T[2], rel=1e-13) and Tn[2, 2] == pytest.approx(T[3], rel=1e-12)
    Pk = cs.nodepressures(P, 3)
    assert len(Pk) == 21 and Pk[0] == P[0] and Pk[2] == P[1] and Pk[1] == P[0] + (P[1] - P[0]) * 0.5
    assert np.array_equal(cs.nodevalues(Tn, 3)[[0, 2, 4]], [Tn[0, 0], Tn[2, 0], Tn[2, 1]])


def test_absorber_validation(cs, lines):
    nu = np.linspace(600, 700, 11)
    g1 = cs.DirectGas(lines("CO2"), 400e-6, nu)
    with pytest.raises(AssertionError):
        cs.UnifiedAbsorber(g1, g1)                       # duplicate absorbers
    with pytest.raises(ValueError):
        cs.UnifiedAbsorber(lambda v, T, P: 0.0)          # needs a gas for the wavenumber grid
    with pytest.raises(AssertionError):
        cs.UnifiedAbsorber(g1, cs.GrayGas(1e-25, nu[:-1]))   # identical wavenumber vectors required
    with pytest.raises(AssertionError):
        cs.DirectGas(lines("CO2"), 1.5, nu)              # concentration in [0,1]
    with pytest.raises(AssertionError):
        cs.DirectGas(lines("CO2"), 1e-4, nu[::-1])       # ascending wavenumbers
    U = cs.UnifiedAbsorber(g1, cs.GrayGas(1e-26, nu), lambda v, T, P: 0 * v)
    assert U.nnu == 11 and len(U.gas) == 2 and len(U.fun) == 1
    assert g1.mu == pytest.approx(np.sum(lines("CO2").A * lines("CO2").mu) / np.sum(lines("CO2").A))


def test_balanced_ranges(cs):
    import workloads as W
    cfg = W.config("C2", nnu=3000)
    for n in (1, 2, 3, 8):
        r = W.balanced_ranges(cfg["nu"], cfg["absorbers"], n)
        assert r[0][0] == 0 and r[-1][1] == 3000 and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all(b > a for a, b in r)


def test_missing_library_fails_loudly(cs, monkeypatch, tmp_path):
    import importlib
    lib_mod = importlib.import_module("clearsky_jl_amd._lib")
    monkeypatch.setattr(lib_mod, "_lib", None)
    monkeypatch.setattr(lib_mod, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(cs.ClearSkyHIPError, match="no CPU fallback"):
        lib_mod.lib()


def test_phco2_plan_host_logic(cs):
    """cs_phco2_plan is pure host code: which interval sizes PHCO2's far wings use, with how many Chebyshev nodes and for which
    chi-regions.  A region is carried at a size while it can hold lines there (30 - 3, 120 - 30, cut-off - 120 cm^-1 minus the
    interval's width); the node count follows from the distance in half-widths h: rho = x0 + sqrt(x0^2 - 1), x0 = 1 + dist / h, and
    (n - 1) log10(rho) >= 18 for n = 16, 32, else 64."""
    nu = np.linspace(1, 2500, 100000)                     # the bench grid: 0.025 cm^-1 per point
    plan = cs.phco2_plan(nu, 500.0)
    assert [p[0] for p in plan] == sorted((p[0] for p in plan), reverse=True) and plan[0][0] == 8192 and plan[-1][0] == 128
    by = {}
    for size, n, regions in plan:
        for r in regions:
            assert (size, r) not in by
            by[(size, r)] = n
    # region 3 (>= 120 cm^-1 away) everywhere, on 32 nodes down to 2048 points and 16 below; region 2 from 2048 points on; region 1
    # from 512 points on, never on 16 nodes (3 cm^-1 is only 1.9 half-widths of a 128-point interval)
    assert {s for (s, r) in by if r == 3} == {8192, 4096, 2048, 1024, 512, 256, 128}
    assert [by[(s, 3)] for s in (8192, 4096, 2048, 1024, 512, 256, 128)] == [32, 32, 32, 16, 16, 16, 16]
    assert {s for (s, r) in by if r == 2} == {2048, 1024, 512, 256, 128} and by[(256, 2)] == 16 and by[(2048, 2)] == 32
    assert {s for (s, r) in by if r == 1} == {512, 256, 128} and by[(512, 1)] == 64 and by[(128, 1)] == 32
    for (size, r), n in by.items():       # the rule itself
        h = 0.5 * (size - 1) * 0.025
        x0 = 1.0 + max({1: 3.0, 2: 30.0, 3: 120.0}[r] / h, 0.3)
        lr = np.log10(x0 + np.sqrt(x0 * x0 - 1.0))
        assert n == (16 if 15 * lr >= 18 else 32 if 31 * lr >= 18 else 64), (size, r, n)
    assert cs.phco2_plan(np.linspace(600, 700, 100), 500.0) == []          # fewer than 128 points: every pair per point
    short = cs.phco2_plan(np.linspace(600, 640, 1601), 500.0)              # 40 cm^-1: no interval larger than the grid / 2
    assert short and max(p[0] for p in short) <= 2048


def test_interp_plan_host_logic(cs):
    """cs_interp_plan is pure host code (no GPU call): interval sizes follow 2.3 N dnu <= 1.5 cut, descending, <= 5 levels."""
    for nu, cut, want in ((np.linspace(1, 2500, 100000), 25.0, [512, 256, 128]),      # the bench grid
                          (np.linspace(1, 2500, 5003), 25.0, []),                      # coarse: every pair evaluated directly
                          (np.linspace(600, 700, 100000), 25.0, [2048, 1024, 512, 256, 128]),
                          (np.linspace(600, 700, 100000), 0.5, [256, 128]),
                          (np.linspace(600, 700, 100), 25.0, []),                      # fewer than 128 points
                          (np.array([667.0]), 25.0, [])):
        got = cs.interp_plan(nu, cut)
        assert got == want, (len(nu), cut, got)
        dnu = (nu[-1] - nu[0]) / max(len(nu) - 1, 1)
        assert all(2.3 * n * dnu <= 1.5 * cut for n in got) and got == sorted(got, reverse=True)
