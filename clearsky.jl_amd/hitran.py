"""HITRAN .par reader, SpectralLines container and the MOLPARAM table (host side, numpy).

Mirrors reference src/hitran/par.jl:1-286 (readpar :91-193, SpectralLines :224-286, ISOINDEX :6-13) and the
data table src/hitran/molparam.jl (extracted to data/molparam.json by tools/gen_molparam.py).
"""
import json
import os
import re
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "molparam.json")
CHEB_LD = 16

# par.jl:6-13
ISOINDEX = {ch: i + 1 for i, ch in enumerate("1234567890ABCDEFGHIJKLMNOPQRSTUVWXYZ")}


@dataclass
class MolParam:
    """par.jl:18-45"""
    M: int
    formula: str
    name: str
    I: list
    isoform: list
    AFGL: list
    A: np.ndarray
    mu: np.ndarray
    Qref: np.ndarray
    hascheb: np.ndarray
    ncheb: np.ndarray
    maxrelerr: np.ndarray
    cheb: list

    def cheb_table(self) -> np.ndarray:
        """[niso, CHEB_LD] row-major table of Chebyshev coefficients (zero padded)."""
        t = np.zeros((len(self.ncheb), CHEB_LD))
        for i, c in enumerate(self.cheb):
            t[i, : len(c)] = c
        return t

    def ncheb_table(self) -> np.ndarray:
        """[niso] int32; 0 where hascheb is false (line_shapes.jl:115-120 throws for those)."""
        return np.where(self.hascheb, self.ncheb, 0).astype(np.int32)


def _load_molparam():
    with open(_DATA) as f:
        d = json.load(f)
    mols = {}
    for m in d["molecules"]:
        if m is None:
            continue
        mols[m["M"]] = MolParam(
            M=m["M"], formula=m["formula"], name=m["name"], I=m["I"], isoform=m["isoform"], AFGL=m["AFGL"],
            A=np.array(m["A"], float), mu=np.array(m["mu"], float), Qref=np.array(m["Qref"], float),
            hascheb=np.array(m["hascheb"], bool), ncheb=np.array(m["ncheb"], np.int64),
            maxrelerr=np.array(m["maxrelerr"], float), cheb=[np.array(c, float) for c in m["cheb"]])
    return d["TMIN"], d["TMAX"], mols


TMIN, TMAX, MOLPARAM = _load_molparam()

_FIELDS = ("M", "I", "nu", "S", "A", "gamma_a", "gamma_s", "Epp", "na", "delta_a")


def readpar(filename: str, numin: float = 0.0, numax: float = np.inf, Scut: float = 0.0, I: Sequence = (),
            maxlines: int = -1, native: bool = True) -> dict:
    """Read a HITRAN 160-column .par file (par.jl:91-193; columns :131-149).

    Filters (nu range, intensity cut, isotopologues, strongest `maxlines`) and the final stable sort by wavenumber
    follow par.jl:153-191.  Returns a dict of numpy arrays keyed M, I (characters), nu, S, A, gamma_a, gamma_s, Epp,
    na, delta_a.

    A valid file, by the same rule in the native parser (cs_par_parse, include/clearsky_hip.h) and here (native=False):
      - a record ends at LF; one CR directly before that LF belongs to the terminator, record by record; the last record may lack
        a terminator; lines of whitespace only are allowed at the very end of the file and nowhere else;
      - every record has exactly 160 characters -- a stump at the end, a blank line in the middle, a 159- or 161-character record
        are refused with the 1-based record number and the length found;
      - nu, S, A, gamma_a, gamma_s, Epp, na, delta_a (columns 4-15, 16-25, 26-35, 36-40, 41-45, 46-55, 56-59, 60-67): blanks trimmed on
        both sides, the whole remainder a plain decimal literal (optional sign, digits with an optional point, optional e/E exponent
        with optional sign) with a finite value; M (columns 1-2) an integer literal; column 3 one of 1-9, 0, A-Z.  Blank fields,
        '#' fill, "1.234-100", D exponents, hex floats, nan/inf, underscores and trailing junk are refused with record number and
        field name, the first such field in file order of the lowest such record.
    A refused file raises ValueError here and ClearSkyHIPError from the native parser (the reference's parse(Float64, ...)
    throws on every one of these fields, par.jl:127-152).  Accepted values are correctly rounded: float() of the trimmed field, bit for bit, in
    both readers, whatever the locale.
    """
    if not filename.endswith(".par"):
        raise AssertionError("expected file with .par extension, downloaded from https://hitran.org/lbl/")
    par = _readpar_native(filename) if native else None    # cs_par_parse: mmap + threads (include/clearsky_hip.h)
    if par is not None:
        return _filter_sort(par, len(par["nu"]), numin, numax, Scut, I, maxlines)
    with open(filename, "rb") as f:
        raw = _records(f.read())
    N = len(raw)
    par = dict(M=np.zeros(N, np.int16), I=np.empty(N, "U1"), nu=np.zeros(N), S=np.zeros(N), A=np.zeros(N),
               gamma_a=np.zeros(N), gamma_s=np.zeros(N), Epp=np.zeros(N), na=np.zeros(N), delta_a=np.zeros(N))
    for i, ln in enumerate(raw):
        par["M"][i] = _field(ln, i, "M", 1, 2, _INTEGER, int)
        if chr(ln[2]) not in ISOINDEX:
            raise ValueError(f"record {i + 1}: field I (columns 3-3) = {ln[2:3]!r} is not an isotopologue character (1-9, 0, A-Z)")
        par["I"][i] = chr(ln[2])
        for name, a, b in _COLUMNS:
            par[name][i] = _field(ln, i, name, a, b, _DECIMAL, float)
    return _filter_sort(par, N, numin, numax, Scut, I, maxlines)


# the numeric fields in file order: columns a..b (1-based, inclusive), par.jl:133-140
_COLUMNS = (("nu", 4, 15), ("S", 16, 25), ("A", 26, 35), ("gamma_a", 36, 40), ("gamma_s", 41, 45), ("Epp", 46, 55), ("na", 56, 59),
            ("delta_a", 60, 67))
_DECIMAL = re.compile(rb"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?")
_INTEGER = re.compile(rb"[+-]?[0-9]+")


def _records(data: bytes) -> list:
    """The layout half of readpar's rule: the 160-character records of a file's bytes, without their terminators."""
    out, pos = [], 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        end = len(data) if nl < 0 else nl
        ln = data[pos:end]
        if nl >= 0 and ln.endswith(b"\r"):
            ln = ln[:-1]
        if len(ln) != 160:
            if not data[pos:].strip(b" \t\n\v\f\r"):
                break   # blank lines at the end of the file
            raise ValueError(f"record {len(out) + 1} has {len(ln)} characters, a HITRAN .par record has 160")
        out.append(ln)
        pos = end + 1
    if not out:
        raise ValueError("the file holds no records")
    return out


def _field(ln, i, name, a, b, literal, convert):
    """The field half: columns a..b of record i (0-based), blanks trimmed, the whole remainder a literal with a finite value."""
    txt = ln[a - 1:b].strip(b" ")
    v = convert(txt) if literal.fullmatch(txt) else np.inf
    if not np.isfinite(v):
        kind = "an integer literal" if convert is int else "a finite plain decimal literal"
        raise ValueError(f"record {i + 1}: field {name} (columns {a}-{b}) = {ln[a - 1:b]!r} is not {kind}")
    return v


def _readpar_native(filename):
    """Parsing loop in the native library (cs_par_parse: mmap + threads); None when the library is not built."""
    import ctypes as C
    from . import _lib
    if not os.path.exists(_lib.LIB_PATH):
        return None
    L = _lib.lib()
    n = C.c_int64()
    _lib.check(L.cs_par_count(filename.encode(), C.byref(n)))
    N = n.value
    par = dict(M=np.zeros(N, np.int16), I=np.zeros(N, "S1"), nu=np.zeros(N), S=np.zeros(N), A=np.zeros(N),
               gamma_a=np.zeros(N), gamma_s=np.zeros(N), Epp=np.zeros(N), na=np.zeros(N), delta_a=np.zeros(N))
    d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    _lib.check(L.cs_par_parse(filename.encode(), N, par["M"].ctypes.data_as(C.POINTER(C.c_int16)),
                              par["I"].ctypes.data_as(C.c_char_p), d(par["nu"]), d(par["S"]), d(par["A"]), d(par["gamma_a"]),
                              d(par["gamma_s"]), d(par["Epp"]), d(par["na"]), d(par["delta_a"])))
    par["I"] = par["I"].astype("U1")
    return par


def _filter_sort(par, N, numin, numax, Scut, I, maxlines):
    """par.jl:153-191: masks, strongest-N selection, stable sort by wavenumber"""
    mask = (par["nu"] >= numin) & (par["nu"] <= numax) & (par["S"] >= Scut)
    if len(I) > 0:
        keep = set(I)
        for j in range(N):
            ch = par["I"][j]
            if (ch not in keep) and (ISOINDEX[ch] not in keep):
                mask[j] = False
    if not mask.any():
        raise AssertionError("par information has been filtered to nothing!")
    par = {k: v[mask] for k, v in par.items()}
    if maxlines > 0 and N > maxlines:  # par.jl:177-186 (N is the unfiltered count there too)
        idx = np.argsort(par["S"], kind="stable")[::-1][:maxlines]
        par = {k: v[idx] for k, v in par.items()}
    idx = np.argsort(par["nu"], kind="stable")
    return {k: v[idx] for k, v in par.items()}


class SpectralLines:
    """Line table of a single gas, sorted by wavenumber (par.jl:224-286).

    Fields (reference names in brackets): name, formula, N, M, I [I], mu [mu], A [A], nu [nu], S, gamma_a [gamma_a],
    gamma_s [gamma_s], Epp, na.  `SpectralLines(filename, **kw)` reads a .par file; `SpectralLines(par_dict)` wraps
    the output of readpar.  The pressure-shift column is kept as delta_a (the reference drops it, quirk 2): the shapes take it with
    pressure_shift=True, through the native parser (Context.load_par, or the file a SpectralLines was read from).
    """

    def __init__(self, src, **kwargs):
        par = readpar(src, **kwargs) if isinstance(src, str) else src
        self.source = (src, dict(kwargs)) if isinstance(src, str) else None   # (a use with pressure_shift=True loads the file natively)
        nu = np.asarray(par["nu"], float)
        N = len(nu)
        Ms = np.unique(par["M"])
        if len(Ms) != 1:
            raise AssertionError("SpectralLines objects must contain only one molecule's lines")
        M = int(Ms[0])
        mp = MOLPARAM[M]
        I = np.array([ISOINDEX[str(c)] if not isinstance(c, (int, np.integer)) else int(c) for c in par["I"]],
                     dtype=np.int16)
        idx = np.argsort(nu, kind="stable")
        self.name, self.formula, self.N, self.M = mp.name, mp.formula, N, M
        self.I = I[idx]
        self.mu = mp.mu[self.I - 1].astype(float)
        self.A = mp.A[self.I - 1].astype(float)
        self.nu = np.ascontiguousarray(nu[idx])
        self.S = np.ascontiguousarray(np.asarray(par["S"], float)[idx])
        self.gamma_a = np.ascontiguousarray(np.asarray(par["gamma_a"], float)[idx])
        self.gamma_s = np.ascontiguousarray(np.asarray(par["gamma_s"], float)[idx])
        self.Epp = np.ascontiguousarray(np.asarray(par["Epp"], float)[idx])
        self.na = np.ascontiguousarray(np.asarray(par["na"], float)[idx])
        # air pressure shift [cm^-1/atm] (par.jl:80,140), used by shapes called with pressure_shift=True; None where the source has none
        self.delta_a = np.ascontiguousarray(np.asarray(par["delta_a"], float)[idx]) if "delta_a" in par else None
        self.ncheb = mp.ncheb_table()
        self.cheb = mp.cheb_table()

    # aliases with the reference's Greek field names
    ν = property(lambda s: s.nu)
    γa = property(lambda s: s.gamma_a)
    γs = property(lambda s: s.gamma_s)
    μ = property(lambda s: s.mu)

    @classmethod
    def synthetic(cls, M: int, L: int, seed: int, numin=0.0, numax=2525.0, iso: int = 1):
        """Seeded synthetic table (SURVEY.md 8d "Lines, C3/C4"): nu ~ U sorted, log10 S ~ U(-28,-19),
        gamma_a ~ U(.05,.10), gamma_s ~ U(.06,.13), E'' ~ U(0,3000), na ~ U(.6,.8), isotopologue `iso`."""
        rng = np.random.Generator(np.random.PCG64(seed))
        par = dict(M=np.full(L, M, np.int16), I=np.full(L, iso, np.int16), nu=np.sort(rng.uniform(numin, numax, L)),
                   S=10.0 ** rng.uniform(-28, -19, L), gamma_a=rng.uniform(0.05, 0.10, L),
                   gamma_s=rng.uniform(0.06, 0.13, L), Epp=rng.uniform(0, 3000, L), na=rng.uniform(0.6, 0.8, L))
        return cls(par)

    def __repr__(self):
        return f"SpectralLines({self.formula}, {self.N} lines, {self.nu[0]:.3f}-{self.nu[-1]:.3f} cm^-1)"
