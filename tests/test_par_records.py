"""The .par readers on records that are not perfect: cs_par_parse / cs_par_count (mmap + threads) and the Python mirror readpar(native=False)
under the one rule for a valid file stated at cs_par_parse (include/clearsky_hip.h) and in readpar's docstring.

Well-formed variants (tests/par_files.py: terminators LF, CRLF and mixed record by record, no final terminator, trailing blank lines, one
record, every isotopologue character of CO2, fields at either end of their columns, signs, exponent spellings, subnormals, a 12-character
wavenumber without an exact double): native = Python = the values the file was written from, all ten fields, bit for bit (-0.0 is not
0.0).  The reference for a value is Python's float() of the trimmed field, which rounds correctly; so does the native parser, 2 000
seeded random strings per field.  Malformed files: both readers refuse every one and name the same 1-based record and the same field
(or the length found).  A file refused for its layout leaves the caller's arrays untouched; one refused for a field leaves unspecified
values in elements 0 .. n-1 and nothing outside them (par_files.native_parse holds both, and that cs_par_count refuses exactly the
layouts cs_par_parse refuses, on every file of this module).  The threaded split of cs_par_parse (from 40 000 records) runs on a
65 000-record file: three threads by thread_count (csrc/cs_par.h) where the machine has them.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import par_files as PF
from conftest import HITRAN


BASE = PF.fixture_records(HITRAN, "CO2", 0, 50)
WELL_FORMED = PF.well_formed(BASE)
MALFORMED = PF.malformed(BASE)


@pytest.fixture(scope="module")
def base():
    return BASE


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("par_records")


def python_table(cs, path):
    """the Python reader's table: every record (no limits), in readpar's stable order by wavenumber"""
    return cs.readpar(str(path), numin=-np.inf, Scut=-np.inf, native=False)


def check_equal(got, want, what):
    for k in PF.FIELDS:
        assert got[k].dtype == want[k].dtype and PF.same(got[k], want[k]), (what, k, got[k], want[k])


def test_the_helper_writes_what_it_says(base):
    """the premises of the files below: 160-character records of molecule 2, a defect lands in its columns, a terminator per record"""
    assert len(base) == 50 and all(len(r) == 160 and r[:2] == " 2" for r in base)
    r = PF.with_defect(base, 16, PF.COLS["S"], " 1.234-100")
    assert r[16][15:25] == " 1.234-100" and r[16][:15] == base[16][:15] and r[16][25:] == base[16][25:] and r[15] == base[15] and base[16] != r[16]
    assert PF.join(["a", "b", "c"], term=["\n", "\r\n", "\n"]) == b"a\nb\r\nc\n" and PF.join(["a", "b"], term="\r\n", last=False, tail="\n") == b"a\r\nb\n"
    assert len(PF.text_record()) == len(PF.text_record("l", nu="9007199254.7")) == 160
    v = PF.values([PF.text_record("l", S="4.941E-324", delta_a="-0.0")])
    assert v["S"][0] == 5e-324 and np.signbit(v["delta_a"][0]) and v["M"][0] == 2 and v["I"][0] == "1" and v["nu"][0] == 667.38
    names = [m[0] for m in MALFORMED] + [w[0] for w in WELL_FORMED]
    assert len(set(names)) == len(names) and len(MALFORMED) >= 30


@pytest.mark.parametrize("name,data,want", WELL_FORMED, ids=[w[0] for w in WELL_FORMED])
def test_well_formed_variant(cs, tmp, name, data, want):
    f = PF.write(tmp / (name + ".par"), data)
    got = PF.native_parse(cs, f)                                         # file order, as a C caller gets it
    check_equal(got, want, "native, file order")
    srt = PF.in_wavenumber_order(want)
    check_equal(python_table(cs, f), srt, "python")
    check_equal(cs.readpar(f, native=True), srt, "native through readpar")


def test_the_variants_hold_what_they_are_for():
    v = dict((n, w) for n, _, w in WELL_FORMED)
    assert v["right_justified"]["nu"][-1] == 9007199254.7 == v["left_justified"]["nu"][-1]
    assert v["right_justified"]["S"][5] == 5e-324 and v["right_justified"]["A"][5] == 2.5e-320        # (subnormals, correctly rounded)
    assert "".join(v["isotopologues"]["I"]) == "1234567890AB"
    assert np.array_equal(v["crlf"]["nu"], v["lf"]["nu"]) and len(v["single"]["nu"]) == 1


def random_field(rng, w):
    """a valid field of at most w characters: fixed or scientific notation, any sign spelling, digits anywhere the grammar allows them"""
    while True:
        sign = rng.choice(["", "", "-", "+"])
        nd = int(rng.integers(1, w + 1))
        digits = "".join(rng.choice(list("0123456789"), nd))
        point = int(rng.integers(0, nd + 2))                             # nd + 1: no point at all
        mant = digits if point > nd else digits[:point] + "." + digits[point:]
        expo = ""
        if rng.random() < 0.5:
            expo = rng.choice(["e", "E"]) + rng.choice(["", "-", "+"]) + str(int(rng.integers(0, 330)))
        t = sign + mant + expo
        if len(t) <= w and np.isfinite(float(t)):
            return t.rjust(w) if rng.random() < 0.5 else t.ljust(w) if rng.random() < 0.5 else t.center(w)


def test_values_are_correctly_rounded(cs, tmp):
    """2 000 seeded random strings in each of the eight numeric fields (widths 12, 10, 5, 4 and 8): native = float() of the trimmed
    field = Python reader, by their bits"""
    rng = np.random.default_rng(20240607)
    recs = []
    for j in range(2000):
        f = {k: random_field(rng, PF.COLS[k][1] - PF.COLS[k][0] + 1) for k in PF.FIELDS[2:]}
        r = PF.text_record(**f)
        for k in PF.FIELDS[2:]:
            r = PF.with_defect([r], 0, PF.COLS[k], f[k])[0]              # (as drawn: text_record would justify it again)
        recs.append(r)
    want = PF.values(recs)
    tiny = np.abs(want["S"])
    assert len(np.unique(want["S"])) > 1500 and np.any((tiny > 0) & (tiny < 2.2e-308)) and np.any(want["nu"] > 1e200)   # (subnormals; large)
    f = PF.write(tmp / "random.par", PF.join(recs))
    check_equal(PF.native_parse(cs, f), want, "native")
    check_equal(python_table(cs, f), PF.in_wavenumber_order(want), "python")


@pytest.mark.parametrize("name,data,record,what", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_file_is_refused_by_both_readers(cs, tmp, name, data, record, what):
    f = PF.write(tmp / (name + ".par"), data)
    pat = PF.refusal_pattern(record, what)
    with pytest.raises(PF.Refused, match=pat):
        PF.native_parse(cs, f)
    with pytest.raises(ValueError, match=pat):
        python_table(cs, f)
    with pytest.raises(cs.ClearSkyHIPError, match=pat):                   # (what a Python caller of the native parser sees)
        cs.readpar(f)
    with pytest.raises(ValueError, match=pat):
        cs.SpectralLines(f, native=False)


def test_refusals_name_the_file(cs, base, tmp):
    f = PF.write(tmp / "named.par", PF.join(PF.with_defect(base, 4, PF.COLS["S"], " 1.234-100")))
    with pytest.raises(PF.Refused, match=r"^record 5: field S \(columns 16-25\) = ' 1.234-100' is not .* \(" + re.escape(f) + r"\)$"):
        PF.native_parse(cs, f)
    f = PF.write(tmp / "blanks_only.par", b"\n  \n\r\n")
    with pytest.raises(PF.Refused, match="no records"):
        PF.native_parse(cs, f)
    with pytest.raises(ValueError, match="no records"):
        python_table(cs, f)


N_BIG = 65000


@pytest.fixture(scope="module")
def big(base, tmp):
    """65 000 records (10 MB): the 50 fixture records over and over, each with a wavenumber of its own"""
    recs = [base[i % 50][:3] + f"{0.01 * i + 0.005:12.6f}" + base[i % 50][15:] for i in range(N_BIG)]
    data = PF.join(recs)
    assert len(data) == N_BIG * 161
    return recs, data, PF.write(tmp / "big.par", data)


def test_threaded_split_against_the_python_reader(cs, base, big):
    recs, data, f = big
    n = ctypes.c_int64()
    assert cs.lib().cs_par_count(f.encode(), ctypes.byref(n)) == 0 and n.value == N_BIG
    assert N_BIG // 20000 == 3                                           # thread_count: min(hardware threads, 32, n / 20000)
    got = PF.native_parse(cs, f)
    assert np.array_equal(got["nu"], np.array([float(r[3:15]) for r in recs])) and np.all(np.diff(got["nu"]) > 0)
    check_equal(got, python_table(cs, f), "threaded")                    # (ascending wavenumbers: the Python table is in file order too)
    for k in PF.FIELDS:
        if k != "nu":
            assert PF.same(got[k], np.tile(PF.values(base)[k], N_BIG // 50)), k


# (0-based records, field, text) -> the 1-based record and field reported; the thirds of the file are the three threads' shares
THREAD_DEFECTS = [
    ([(10000, "S", " 1.234-100")], 10001, "S"),
    ([(30000, "nu", "  ##########")], 30001, "nu"),
    ([(60000, "Epp", "       1_0")], 60001, "Epp"),
    ([(60000, "S", " " * 10), (30000, "gamma_a", "  nan")], 30001, "gamma_a"),
    ([(10000, "I", " "), (64999, "S", " " * 10)], 10001, "I"),
    ([(43333, "M", "2."), (43332, "na", "   -"), (21666, "delta_a", "       ."), (21665, "A", "1.000E+00x")], 21666, "A"),   # at the share edges
    ([(64999, "delta_a", "   1.0E-")], 65000, "delta_a"),
]


@pytest.mark.parametrize("case", range(len(THREAD_DEFECTS)))
def test_threads_report_the_lowest_record(cs, big, tmp, case):
    recs, data, _ = big
    defects, record, fld = THREAD_DEFECTS[case]
    d = bytearray(data)
    for i, k, text in defects:
        a, b = PF.COLS[k]
        assert len(text) == b - a + 1
        d[161 * i + a - 1:161 * i + b] = text.encode()
    assert len(d) == len(data)
    f = PF.write(tmp / f"big_defect{case}.par", bytes(d))
    pat = PF.refusal_pattern(record, fld)
    with pytest.raises(PF.Refused, match=pat):
        PF.native_parse(cs, f)
    if record < 25000:                                                   # (the Python reader stops there too; further in it only takes longer)
        with pytest.raises(ValueError, match=pat):
            python_table(cs, f)
    os.remove(f)


def test_layout_refusals_in_a_long_file(cs, big, tmp):
    """the index pass of a file long enough for threads: a record one character short far in, and a blank line there"""
    recs, data, _ = big
    for name, d, length in (("short", data[:161 * 50000 + 159] + data[161 * 50000 + 160:], 159),
                            ("blank", data[:161 * 50000] + b"\n" + data[161 * 50000:], 0)):
        f = PF.write(tmp / f"big_{name}.par", d)
        with pytest.raises(PF.Refused, match=PF.refusal_pattern(50001, length)):
            PF.native_parse(cs, f)
        os.remove(f)


def test_count_and_parse_disagree_with_the_caller(cs, base, tmp):
    """cs_par_parse with another n than the file's: refused, arrays as they were"""
    f = PF.write(tmp / "fifty.par", PF.join(base))
    a = np.full(60, 7.0)
    dp = ctypes.POINTER(ctypes.c_double)
    p = a.ctypes.data_as(dp)
    M, I = np.zeros(60, np.int16), np.zeros(60, "S1")
    for n in (49, 51):
        rc = cs.lib().cs_par_parse(f.encode(), n, M.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), I.ctypes.data_as(ctypes.c_char_p), p, p, p, p, p, p, p, p)
        assert rc == -1 and "file holds 50 records, caller expects %d" % n in cs.lib().cs_last_error().decode()
        assert np.all(a == 7.0) and not M.any()
