"""HITRAN .par files written by the tests: whole tables (`write_par`), single records from field texts (`text_record`), one defect in one
record (`with_defect`), a terminator per record (`join`) -- and the two things tests/test_par_records.py and tests/test_gpu_par_load.py
share: the well-formed variants with the values they were written from (`well_formed`) and the malformed files with the record and field
a reader has to name (`malformed`).  The rule itself is stated at cs_par_parse (include/clearsky_hip.h) and in readpar's docstring.
"""
import ctypes
import os
import re

import numpy as np

FIELDS = ("M", "I", "nu", "S", "A", "gamma_a", "gamma_s", "Epp", "na", "delta_a")
# columns a..b of each field, 1-based and inclusive (par.jl:131-140)
COLS = {"M": (1, 2), "I": (3, 3), "nu": (4, 15), "S": (16, 25), "A": (26, 35), "gamma_a": (36, 40), "gamma_s": (41, 45), "Epp": (46, 55),
        "na": (56, 59), "delta_a": (60, 67)}
ISOCHAR = {1: "1", 2: "2", 3: "3", 4: "4", 5: "5", 6: "6", 7: "7", 8: "8", 9: "9", 10: "0", 11: "A", 12: "B"}


def _fx(x, w, dec):
    """x in a fixed field of w characters with dec decimals (HITRAN drops the leading zero where the field needs it: .0927, -.23)"""
    r = f"{x:.{dec}f}"
    if len(r) > w:
        r = r.replace("0.", ".", 1)
    assert len(r) <= w, (x, w)
    return r.rjust(w)


def write_par(path, M, nu, S, ga, gs, Epp, na, da, iso=None):
    """a HITRAN 160-column file of these lines (par.jl:131-149 layout); read back through the parser, its values are the table's"""
    iso = np.ones(len(nu), int) if iso is None else iso
    with open(path, "w") as f:
        for j in range(len(nu)):
            r = (f"{M:2d}{ISOCHAR[int(iso[j])]}{nu[j]:12.6f}{S[j]:10.3E}{1.0:10.3E}{_fx(ga[j], 5, 4)}{_fx(gs[j], 5, 3)}{Epp[j]:10.4f}"
                 f"{_fx(na[j], 4, 2)}{_fx(da[j], 8, 5)}")
            assert len(r) == 67, r
            f.write(r + " " * 93 + "\n")
    return str(path)


# ---- records as text ------------------------------------------------------------------------------------------------------------

DEFAULT = dict(M="2", I="1", nu="667.380000", S="1.000E-20", A="1.000E+00", gamma_a=".0750", gamma_s="0.100", Epp="100.0000", na="0.75",
               delta_a="-.00100")


def text_record(just="r", **fields):
    """one 160-character record from field TEXTS, each right- ("r") or left-justified ("l") inside its columns; fields not given: DEFAULT"""
    r = ""
    for name in FIELDS:
        a, b = COLS[name]
        t = str(fields.get(name, DEFAULT[name]))
        assert len(t) <= b - a + 1, (name, t)
        r += t.rjust(b - a + 1) if just == "r" else t.ljust(b - a + 1)
    return r + " " * 93


def with_defect(records, i, cols, text):
    """a copy of the records with columns cols = (a, b) (1-based, inclusive) of record i (0-based) replaced by `text`"""
    a, b = cols
    assert len(text) == b - a + 1, (cols, text)
    out = list(records)
    out[i] = out[i][:a - 1] + text + out[i][b:]
    return out


def join(records, term="\n", last=True, tail=""):
    """the file's bytes: record i followed by term (one terminator for all) or term[i]; last=False: the last record without its terminator;
    `tail` follows the last record"""
    terms = [term] * len(records) if isinstance(term, str) else list(term)
    assert len(terms) == len(records)
    if not last:
        terms[-1] = ""
    return ("".join(r + t for r, t in zip(records, terms)) + tail).encode("ascii")


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def values(records):
    """the values the records were written from, in file order: Python's int() / float() of each trimmed field (the correctly rounded
    value of the text), I as characters"""
    out = {k: [] for k in FIELDS}
    for r in records:
        for k in FIELDS:
            a, b = COLS[k]
            t = r[a - 1:b].strip(" ")
            out[k].append(int(t) if k == "M" else t if k == "I" else float(t))
    return {k: np.array(v, dtype=np.int16 if k == "M" else "U1" if k == "I" else float) for k, v in out.items()}


def fixture_records(hitran_dir, name="CO2", lo=0, n=50):
    """records lo .. lo+n-1 of a clean fixture under tests/golden/hitran, as text"""
    with open(os.path.join(hitran_dir, name + ".par"), "rb") as f:
        recs = [ln.rstrip(b"\r").decode("ascii") for ln in f.read().split(b"\n") if ln.strip()]
    assert all(len(r) == 160 for r in recs)
    return recs[lo:lo + n]


def bits(a):
    """fp64 arrays by their bits (-0.0 is not 0.0 here), everything else as it is"""
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b)))


def in_wavenumber_order(v):
    """readpar's last step on a table in file order: stable sort by wavenumber (par.jl:188-191)"""
    idx = np.argsort(v["nu"], kind="stable")
    return {k: a[idx] for k, a in v.items()}


# ---- the files -------------------------------------------------------------------------------------------------------------------

def well_formed(base):
    """[(name, file bytes, values in file order)] -- every variant a reader has to accept, on `base` (clean records of one molecule, M = 2)
    and on records written from field texts"""
    n = len(base)
    out = []

    def add(name, records, **kw):
        out.append((name, join(records, **kw), values(records)))

    add("lf", base)
    add("crlf", base, term="\r\n")
    add("crlf_block_in_lf", base, term=["\r\n" if n // 2 - 5 <= i < n // 2 + 5 else "\n" for i in range(n)])   # two downloads concatenated
    add("lf_crlf_alternating", base, term=["\r\n" if i % 3 == 1 else "\n" for i in range(n)])
    add("no_final_lf", base, last=False)
    add("no_final_crlf", base, term="\r\n", last=False)
    add("trailing_blank_lines", base, tail="\n  \r\n\t\n")
    add("trailing_blanks_unterminated", base, tail="   ")
    add("single", base[:1])
    add("single_unterminated", base[:1], last=False)
    add("isotopologues", [text_record(I=c, nu=f"{600 + j}.5") for j, c in enumerate("1234567890AB")])
    texts = [dict(nu="667.5", S="1.5e-21", A="2.5", gamma_a=".07", gamma_s=".1", Epp="3.25", na=".7", delta_a="-.002"),
             dict(nu="668.", S="3.E-22", A="7", gamma_a="1", gamma_s="0", Epp="0.", na="1.", delta_a="0"),
             dict(nu="669.25", na="-.5", delta_a="-.01234"),                                     # negative na and delta_a
             dict(nu="+670.125", S="+1.0E-20", A="+1.0E+00", gamma_a="+.07", gamma_s="+0.1", Epp="+100.5", na="+.75", delta_a="+.00125", M="+2"),
             dict(nu="671.0E+00", S="1.000E+00", A="2.500e-05", Epp="1.5e+03", delta_a="-1.0e-05", M="02"),
             dict(nu="672.000000", S="4.941E-324", A="2.5E-320"),                                # into the subnormals: correct rounding
             dict(nu="673.5", S="1.0E-400", delta_a="-0.0"),                                     # underflow to zero is finite; minus zero
             dict(nu="9007199254.7", S="1.797E+308")]                                            # twelve characters, no exact double
    add("right_justified", [text_record("r", **t) for t in texts])
    add("left_justified", [text_record("l", **t) for t in texts], term="\r\n")
    return out


def malformed(base):
    """[(name, file bytes, record, what)] -- every file both readers have to refuse: `record` is the 1-based number the message names,
    `what` the field name, or the length found for a record that has not 160 characters"""
    n = len(base)
    mid = n // 3           # (0-based; reported as mid + 1)
    out = []

    def field(name, fld, text, i=mid):
        out.append((name, join(with_defect(base, i, COLS[fld], text)), i + 1, fld))

    field("S_exponent_without_letter", "S", " 1.234-100")       # Fortran's three-digit exponent, as E10.3 prints it
    field("S_D_exponent", "S", " 1.234D-20")
    field("S_hex_float", "S", "0x1p-70   ")
    field("S_blank", "S", " " * 10)
    field("nu_hash_fill", "nu", "  ##########")
    field("gamma_a_nan", "gamma_a", "  nan")
    field("gamma_s_inf", "gamma_s", "  inf")
    field("Epp_underscore", "Epp", "       1_0")
    field("A_trailing_junk", "A", "1.000E+00x")
    field("A_two_numbers", "A", " 1.0 2.0  ")
    field("na_sign_only", "na", "   -")
    field("delta_a_point_only", "delta_a", "       .")
    field("delta_a_exponent_without_digits", "delta_a", "   1.0E-")
    field("S_overflow", "S", "  1.0E+999")                       # a plain decimal literal whose value is not finite
    field("nu_tab_inside", "nu", "  667.38\t   ")
    field("M_with_point", "M", "2.")
    field("M_blank", "M", "  ")
    field("I_space", "I", " ")
    field("I_lower_case", "I", "a")
    field("first_record", "S", " " * 10, i=0)
    field("last_record", "S", " " * 10, i=n - 1)
    out.append(("two_fields_of_one_record", join(with_defect(with_defect(base, mid, COLS["na"], "    "), mid, COLS["A"], " " * 10)), mid + 1, "A"))
    out.append(("two_records", join(with_defect(with_defect(base, n - 2, COLS["nu"], " " * 12), 3, COLS["Epp"], " " * 10)), 4, "Epp"))
    out.append(("161_characters", join(base[:mid] + [base[mid] + " "] + base[mid + 1:]), mid + 1, 161))
    out.append(("159_characters", join(base[:mid] + [base[mid][:-1]] + base[mid + 1:]), mid + 1, 159))
    out.append(("159_characters_crlf", join(base[:mid] + [base[mid][:-1]] + base[mid + 1:], term="\r\n"), mid + 1, 159))
    out.append(("cr_cr_lf", join(base[:mid] + [base[mid] + "\r"] + base[mid + 1:], term="\r\n"), mid + 1, 161))
    out.append(("blank_line_in_the_middle", join(base[:mid] + [""] + base[mid:]), mid + 1, 0))
    out.append(("whitespace_line_in_the_middle", join(base[:mid] + ["   "] + base[mid:]), mid + 1, 3))
    out.append(("blank_first_line", join([""] + base), 1, 0))
    out.append(("cut_off_inside_the_last_record", join(base, tail=base[0][:100]), n + 1, 100))
    out.append(("cut_off_after_cr", join(base, term="\r\n", last=False, tail="\r"), n, 161))
    return out


def refusal_pattern(record, what):
    """what a refusal has to say, in either reader: the 1-based record number and the field name or the length found"""
    if isinstance(what, int):
        return rf"record {record} has {what} characters"
    return rf"record {record}: field {what}\b"


# ---- the native parser, called as a C program would --------------------------------------------------------------------------------

GUARD = 8   # elements on either side of the arrays handed to cs_par_parse that it must leave alone


class Refused(Exception):
    pass


def native_parse(cs, path, fill=None):
    """cs_par_count, then cs_par_parse into the middle of arrays that carry GUARD elements on either side: the table in file order.
    Refusals raise Refused with the library's message.  Held on every file that goes through here: cs_par_count refuses exactly the
    files cs_par_parse refuses for their layout, with the same message; a layout refusal leaves the arrays untouched; a field refusal
    leaves the guards untouched."""
    L = cs.lib()
    f = str(path).encode()
    n = ctypes.c_int64(-1)
    rc_count = L.cs_par_count(f, ctypes.byref(n))
    msg_count = L.cs_last_error().decode() if rc_count else None
    N = n.value if rc_count == 0 else 64     # (a refused count: parse is still asked, with arrays it must not touch)
    rng = np.random.default_rng(5)
    arr = {"M": rng.integers(-999, 999, N + 2 * GUARD).astype(np.int16), "I": np.full(N + 2 * GUARD, b"~", "S1")}
    for k in FIELDS[2:]:
        arr[k] = rng.standard_normal(N + 2 * GUARD)
    before = {k: a.copy() for k, a in arr.items()}
    dp = ctypes.POINTER(ctypes.c_double)
    ptr = lambda k, t: ctypes.cast(arr[k][GUARD:].ctypes.data, t)
    rc = L.cs_par_parse(f, N, ptr("M", ctypes.POINTER(ctypes.c_int16)), ptr("I", ctypes.c_char_p), *[ptr(k, dp) for k in FIELDS[2:]])
    msg = L.cs_last_error().decode() if rc else None
    for k in FIELDS:
        assert same(arr[k][:GUARD], before[k][:GUARD]) and same(arr[k][-GUARD:], before[k][-GUARD:]), ("guard", k)
    if rc_count:
        assert rc == rc_count == -1 and msg == msg_count and re.search(r"record \d+ has \d+ characters|holds no records", msg), (msg_count, msg)
        assert all(same(arr[k], before[k]) for k in FIELDS), "a layout refusal must leave the arrays untouched"
        raise Refused(msg)
    if rc:
        assert rc == -1 and re.search(r"record \d+: field \w+", msg), msg
        raise Refused(msg)
    out = {k: arr[k][GUARD:GUARD + N].copy() for k in FIELDS}
    out["I"] = out["I"].astype("U1")
    return out
