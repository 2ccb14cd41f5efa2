""".par files straight into a gas slot (Context.load_par / cs_gas_upload_par) under the rule for a valid file (cs_par_parse,
include/clearsky_hip.h), on the files of tests/par_files.py and tables of a few hundred lines.

  - every well-formed variant: what cs_gas_fetch returns from the slot is the table the file was written from, bit for bit (stable order
    by wavenumber, isotopologue numbers through ISOINDEX, molar masses from MOLPARAM), and one flagged Voigt evaluation of the
    mixed-terminator file shows that the file's own delta_a went along (tests/test_gpu_pressure_shift.py's expected values at its 1e-9
    for arbitrary shifts and pressures -- measured 4e-16 and 9e-16; the unshifted sum is 3e-3 and 7e-3 away);
  - every malformed file onto a slot that holds a table: ClearSkyHIPError with record and field, the slot's table and its shifts as they
    were, and the context has lost no slot;
  - the filters on a table with ties (equal wavenumbers across isotopologues, equal intensities on both sides of the maxlines boundary,
    limits that equal a record's value, isotopologues as integers, characters and both, maxlines below the filtered count, between it
    and N -- the reference selects whenever the UNFILTERED count exceeds maxlines -- and above N): the slot against the Python mirror
    SpectralLines(f, **kw) and against `restated`, par.jl:153-191 written out here.
"""
import ctypes as C

import numpy as np
import pytest

import par_files as PF
import test_gpu_pressure_shift as PS
from conftest import HITRAN

pytestmark = pytest.mark.gpu

M_CO2 = 2
NAMES = ("nu", "S", "gamma_a", "gamma_s", "Epp", "na", "mu")


@pytest.fixture(scope="module")
def ctx(cs):
    c = cs.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("par_load")


@pytest.fixture(scope="module")
def base():
    """300 CO2 records of the 15 um band"""
    recs = PF.fixture_records(HITRAN, "CO2", 0, 10 ** 9)
    lo = int(np.searchsorted(PF.values(recs)["nu"], 640.0))
    return recs[lo:lo + 300]


def fetch(cs, ctx, slot, n):
    """the slot's table as cs_gas_fetch returns it"""
    out = {k: np.full(n, np.nan) for k in NAMES}
    iso = np.full(n, -1, np.int16)
    cs.check(cs.lib().cs_gas_fetch(ctx.handle, slot, n, *[cs.dptr(out[k]) for k in NAMES], iso.ctypes.data_as(C.POINTER(C.c_int16))))
    out["iso"] = iso
    return out


def slot_table(cs, v):
    """what the slot has to hold for the records `v` (already filtered, any order): stable order by wavenumber, ISOINDEX, MOLPARAM's mu"""
    v = PF.in_wavenumber_order(v)
    iso = np.array(["1234567890ABCDEFGHIJKLMNOPQRSTUVWXYZ".index(c) + 1 for c in v["I"]], np.int16)
    out = {k: v[k] for k in NAMES[:-1]}
    out["mu"] = np.asarray(cs.MOLPARAM[M_CO2].mu, float)[iso - 1]
    out["iso"] = iso
    return out


def check_slot(got, want, what):
    for k in want:
        assert PF.same(got[k], want[k]), (what, k)


def test_well_formed_variants_into_a_slot(cs, O, ctx, base, tmp):
    loaded = {}
    for name, data, v in PF.well_formed(base):
        sl = ctx.load_par(PF.write(tmp / (name + ".par"), data), M_CO2)
        want = slot_table(cs, v)
        assert sl.N == len(want["nu"])
        check_slot(fetch(cs, ctx, ctx.slot_of(sl), sl.N), want, name)
        loaded[name] = (sl, PF.in_wavenumber_order(v)["delta_a"])
    # the file's own shifts are attached: one flagged evaluation, 64 points across the table, two states
    sl, da = loaded["crlf_block_in_lf"]
    assert np.count_nonzero(da) > 250
    nu = np.linspace(sl.nu[0] - 0.01, sl.nu[-1] + 0.01, 64)
    T, P, Pp = [296.0, 240.0], [1.7 * PS.KATM, 0.31 * PS.KATM], [500.0, 80.0]
    s = cs.shape_batch(sl, "voigt", nu, T, P, Pp, PS.CUT, ctx, pressure_shift=True)
    for k in range(2):
        r = PS.expected(O, sl, da, "voigt", nu, T[k], P[k], Pp[k], True)
        err = np.max(np.abs(s[k] - r)) / np.max(np.abs(r))
        r0 = PS.expected(O, sl, 0.0 * da, "voigt", nu, T[k], P[k], Pp[k], True)
        print(f"state {k}: flagged sum vs expected {err:.2e}, expected vs unshifted {np.max(np.abs(r - r0)) / np.max(np.abs(r)):.2e}")
        assert err < 1e-9, k
        assert np.max(np.abs(r - r0)) > 1e-4 * np.max(np.abs(r)), k      # (the shifts matter at these states: 1e-9 tells them apart)


def test_refused_file_on_a_filled_slot(cs, base, tmp):
    L = cs.lib()
    ctx = cs.Context(0)
    good = ctx.load_par(PF.write(tmp / "good.par", PF.join(base, term="\r\n")), M_CO2)
    slot = ctx.slot_of(good)
    held = fetch(cs, ctx, slot, good.N)
    check_slot(held, slot_table(cs, PF.values(base)), "good")
    nu = np.linspace(good.nu[0], good.nu[-1], 64)
    state = ([280.0], [0.9 * PS.KATM], [300.0])
    before = cs.shape_batch(good, "voigt", nu, *state, PS.CUT, ctx, pressure_shift=True)
    mp = cs.MOLPARAM[M_CO2]
    mu, ncheb, cheb = cs.as_f64(mp.mu), np.ascontiguousarray(mp.ncheb_table(), dtype=np.int32), cs.as_f64(mp.cheb_table())
    none = np.zeros(1, np.int32)
    cases = PF.malformed(base[:60])
    for name, data, record, what in cases:
        f = PF.write(tmp / (name + ".par"), data)
        pat = PF.refusal_pattern(record, what)
        with pytest.raises(cs.ClearSkyHIPError, match=pat):
            ctx.load_par(f, M_CO2)
        n = C.c_int64(-7)
        rc = L.cs_gas_upload_par(ctx.handle, slot, f.encode(), 0.0, 1e300, 0.0, none.ctypes.data_as(C.POINTER(C.c_int)), 0, -1, M_CO2, cs.dptr(mu),
                                 len(mu), ncheb.ctypes.data_as(C.POINTER(C.c_int32)), cs.dptr(cheb), C.byref(n))
        assert rc == PS.EINVAL and n.value == -7, name
        with pytest.raises(cs.ClearSkyHIPError, match=pat):
            cs.check(rc)
        check_slot(fetch(cs, ctx, slot, good.N), held, name)             # the earlier table, bit for bit
    assert len(cases) > 16                                               # more refusals than a context has slots
    assert np.array_equal(cs.shape_batch(good, "voigt", nu, *state, PS.CUT, ctx, pressure_shift=True), before)   # (its shifts are still there)
    again = ctx.load_par(PF.write(tmp / "again.par", PF.join(base[:7])), M_CO2)
    assert ctx.slot_of(again) == slot + 1 and again.N == 7               # (none of them cost the context a slot)
    ctx.close()


# ---- filters -----------------------------------------------------------------------------------------------------------------------

def tie_table():
    """24 records in shuffled file order: wavenumbers shared by up to three isotopologues, intensities from five values"""
    nu = [600.0, 600.0, 600.0, 601.5, 601.5, 602.25, 603.0, 603.0, 604.5, 605.0, 605.0, 605.0, 606.75, 607.0, 607.0, 608.5, 609.0, 609.0,
          610.0, 610.0, 611.0, 612.0, 612.0, 613.0]
    iso = "123121231124212312341231"
    S = ["1.000E-22", "2.000E-22", "5.000E-22", "1.000E-21", "2.000E-21"]
    rng = np.random.default_rng(11)
    order = rng.permutation(len(nu))
    return [PF.text_record(I=iso[j], nu=f"{nu[j]:.6f}", S=S[int(rng.integers(0, 5))], gamma_a=f".{700 + j:04d}", Epp=f"{100 + j}.5000",
                           delta_a=f"-.{j + 1:05d}") for j in order]


def restated(v, numin=0.0, numax=np.inf, Scut=0.0, I=(), maxlines=-1):
    """par.jl:153-191 on the table v in file order, as record numbers: the masks, the `maxlines` strongest whenever the unfiltered count
    exceeds maxlines (reverse of the stable ascending order), the stable sort by wavenumber"""
    N = len(v["nu"])
    number = {c: j + 1 for j, c in enumerate("1234567890ABCDEFGHIJKLMNOPQRSTUVWXYZ")}
    keep = [j for j in range(N) if numin <= v["nu"][j] <= numax and v["S"][j] >= Scut
            and (len(I) == 0 or v["I"][j] in I or number[v["I"][j]] in I)]
    assert keep, "par information has been filtered to nothing!"
    if maxlines > 0 and N > maxlines:
        keep = sorted(keep, key=lambda j: v["S"][j])[::-1][:maxlines]
    keep = sorted(keep, key=lambda j: v["nu"][j])
    return {k: a[keep] for k, a in v.items()}


FILTERS = [dict(), dict(numin=601.5, numax=610.0), dict(numin=600.0, numax=600.0), dict(Scut=5e-22), dict(Scut=2e-21),
           dict(I=(1, 2)), dict(I=("1", "2")), dict(I=(1, "2")), dict(I=("3", 4)),
           dict(maxlines=1), dict(maxlines=5), dict(maxlines=9), dict(maxlines=14), dict(maxlines=23), dict(maxlines=24), dict(maxlines=100),
           dict(numin=601.5, numax=610.0, maxlines=6), dict(numin=603.0, numax=607.0, I=(1, "2"), maxlines=20),
           dict(numin=601.5, numax=612.0, Scut=2e-22, I=(1, 2, "3"), maxlines=7),
           dict(Scut=5e-22, maxlines=20), dict(I=("1",), maxlines=15), dict(numin=600.0, numax=605.0, maxlines=12)]


def test_filters_on_a_table_with_ties(cs, tmp):
    recs = tie_table()
    v = PF.values(recs)
    N = len(recs)
    assert N == 24 and len(np.unique(v["nu"])) < 16 and len(np.unique(v["S"])) == 5 and np.any(np.diff(v["nu"]) < 0)
    f = PF.write(tmp / "ties.par", PF.join(recs))
    ctx = cs.Context(0)
    straddled = quirk = reordered = 0
    for kw in FILTERS:
        want = restated(v, **kw)
        m = kw.get("maxlines", -1)
        unlimited = restated(v, **{k: x for k, x in kw.items() if k != "maxlines"})
        nf = len(unlimited["nu"])
        if 0 < m < nf:
            Ssorted = np.sort(unlimited["S"])[::-1]
            straddled += Ssorted[m - 1] == Ssorted[m]                    # equal intensities on both sides of the boundary
        if nf <= m < N:
            quirk += 1
            reordered += not PF.same(want["gamma_a"], unlimited["gamma_a"])   # (kept whole, but equal wavenumbers now by descending S)
        a = ctx.load_par(f, M_CO2, **kw)
        check_slot(fetch(cs, ctx, ctx.slot_of(a), a.N), slot_table(cs, want), kw)
        b = cs.SpectralLines(f, native=False, **kw)
        assert a.N == b.N == len(want["nu"])
        for k in NAMES:
            assert PF.same(getattr(a, k), getattr(b, k)), (kw, k)
        assert PF.same(a.I, b.I) and PF.same(b.delta_a, want["delta_a"]), kw
    assert straddled >= 3 and quirk >= 2 and reordered >= 1              # the table does hold the cases the docstring names
    for kw in (dict(numin=613.5), dict(Scut=1e-20), dict(I=(7,))):
        with pytest.raises(cs.ClearSkyHIPError, match="filtered to nothing"):
            ctx.load_par(f, M_CO2, **kw)
        with pytest.raises(AssertionError, match="filtered to nothing"):
            cs.SpectralLines(f, native=False, **kw)
    ctx.close()
