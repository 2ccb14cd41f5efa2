"""Collision-induced absorption: .cia reader, CIATables and the cia() cross-section formula (host side).

Mirrors reference src/absorption/collision_induced_absorption.jl: readcia :39-94, CIATables :145-235, the functor :251-276,
cia :295-303,:318-323.  Inside a Column the tables are evaluated by the k_cia kernel; the numpy paths here serve scalar
calls and tests.

Beyond the reference: `CIATables(..., radiation=True)` (CS_CIA_RADIATION of include/clearsky_hip.h) multiplies the tables' k by the
radiation term R(nu, T) = nu tanh(c2 nu / 2T), and `Continuum` builds such tables from continuum coefficients in MT_CKD form.
"""
import math

import numpy as np

from . import constants as K


def readcia(filename: str):
    """readcia(filename) :39-94 -> list of dicts (symbol, numin, numax, npts, T, maxcia, res, comments, reference, nu, k)"""
    assert filename.endswith(".cia"), "expected file with .cia extension downloaded from https://hitran.org/cia/"
    with open(filename) as f:
        lines = [ln.rstrip("\n").rstrip("\r") for ln in f]
    while lines and lines[-1] == "":
        lines.pop()
    L = [len(ln) for ln in lines]
    assert max(L) == 100, f"unexpected maximum line length in cia file, expected 100 but got {max(L)}"
    hidx = [i for i, n in enumerate(L) if n == 100] + [len(lines)]
    data = []
    for a, b in zip(hidx[:-1], hidx[1:]):
        h = lines[a]
        d = dict(symbol=h[0:20].strip(), numin=float(h[20:30]), numax=float(h[30:40]), npts=int(h[40:47]), T=float(h[47:54]),
                 maxcia=float(h[54:64]), res=float(h[64:70]), comments=h[70:97].strip(), reference=int(h[97:100]))
        rows = [ln.split() for ln in lines[a + 1:b]]
        d["nu"] = np.array([float(r[0]) for r in rows])
        d["k"] = np.array([float(r[1]) for r in rows])
        data.append(d)
    return data


C2 = 100.0 * K.h * K.c / K.k      # 100 h c / k [cm K], line_shapes.jl:5


def radiation_term(nu, T):
    """R(nu, T) = nu tanh(c2 nu / 2T) [cm^-1], formed as the device forms it (exact to rounding as nu -> 0)"""
    return nu * math.tanh(C2 * nu / (2.0 * T))


def cia(*args):
    """cia(k, T, Pa, P1, P2) :295-303  or  cia(nu, tables, T, Pa, P1, P2) :318-323 -> cross-section [cm^2/molecule]"""
    if len(args) == 6:
        nu, x, T, Pa, P1, P2 = args
        return cia(x(nu, T), T, Pa, P1, P2)
    k, T, Pa, P1, P2 = args
    rho1 = (P1 / K.atm) * (K.T0 / T)
    rho2 = (P2 / K.atm) * (K.T0 / T)
    rhoa = 1e-6 * Pa / (K.k * T)
    return (k * K.Lo2) * rho1 * rho2 / rhoa


class CIATables:
    """CIATables(data_or_filename; extrapolate=False, singles=False, radiation=False) :145-242.

    `grids`: list of (nu[nb], T[nt], lnk[nt, nb]) -- bilinear interpolation of ln k (BilinearInterpolator, NoBoundaries);
    `single`: list of (nu, lnk, T) single-temperature ranges (LinearInterpolator).  Callable: tables(nu, T) -> k.
    `radiation`: tables(nu, T) -> R(nu, T) k with R = nu tanh(c2 nu / 2T) at the exact nu and T, on the device as here (the
    tables then hold a k per cm^-1: see Continuum).
    """

    def __init__(self, data, extrapolate: bool = False, singles: bool = False, verbose: bool = False, radiation: bool = False):
        self.filename = data if isinstance(data, str) else None
        if isinstance(data, str):
            data = readcia(data)
        ranges = sorted(set((d["numin"], d["numax"]) for d in data), key=lambda r: r[0])
        self.grids, self.single = [], []
        for lo, hi in ranges:
            sel = [d for d in data if math.isclose(d["numin"], lo) and math.isclose(d["numax"], hi)]
            if len(sel) == 1:
                k = sel[0]["k"].copy()
                k[k <= 0.0] = 0.0
                with np.errstate(divide="ignore"):
                    self.single.append((sel[0]["nu"].copy(), np.log(k), float(sel[0]["T"])))
            else:
                for d in sel[1:]:
                    assert math.isclose(float(np.sum(sel[0]["nu"] - d["nu"])), 0.0, abs_tol=1e-12), \
                        "wavenumber sample within a wavenumber range appear to be different"
                sel = sorted(sel, key=lambda d: d["T"])
                k = np.array([d["k"] for d in sel], dtype=float)         # [nt, nb]
                k[k <= 0.0] = np.finfo(float).tiny
                self.grids.append((sel[0]["nu"].copy(), np.array([d["T"] for d in sel], float), np.log(k)))
        symbols = sorted(set(d["symbol"] for d in data))
        assert len(symbols) == 1
        self.name = symbols[0]
        self.formulae = tuple(self.name.split("-"))
        self.extrapolate, self.singles, self.radiation = bool(extrapolate), bool(singles), bool(radiation)
        if verbose:
            print(f"creating CIATables\n  formulae: {self.formulae[0]} & {self.formulae[1]}\n  {len(self.grids) + len(self.single)} absorption region(s)")

    def __call__(self, nu, T):
        """tables(nu, T) :251-276 (scalar nu)"""
        k = 0.0
        for g_nu, g_T, lnk in self.grids:
            if g_nu[0] <= nu <= g_nu[-1]:
                if g_T[0] <= T <= g_T[-1]:
                    k += math.exp(_bilinear(g_nu, g_T, lnk, nu, T))
                elif self.extrapolate:
                    k += math.exp(_bilinear(g_nu, g_T, lnk, nu, g_T[-1] if T > g_T[-1] else g_T[0]))
        if self.singles:
            for s_nu, s_lnk, _ in self.single:
                if s_nu[0] <= nu <= s_nu[-1]:
                    i = min(max(int(np.searchsorted(s_nu, nu, side="right")) - 1, 0), len(s_nu) - 2)
                    with np.errstate(invalid="ignore"):
                        k += math.exp((nu - s_nu[i]) * (s_lnk[i + 1] - s_lnk[i]) / (s_nu[i + 1] - s_nu[i]) + s_lnk[i])
        if self.radiation:
            k *= radiation_term(nu, T)
        return k

    def __repr__(self):
        return f"CIATables - {self.name}"


def _bilinear(xg, yg, z, x, y):
    i = min(max(int(np.searchsorted(xg, x, side="right")) - 1, 0), len(xg) - 2)
    j = min(max(int(np.searchsorted(yg, y, side="right")) - 1, 0), len(yg) - 2)
    xx = (x - xg[i]) / (xg[i + 1] - xg[i])
    yy = (y - yg[j]) / (yg[j + 1] - yg[j])
    return (1 - xx) * (1 - yy) * z[j, i] + xx * (1 - yy) * z[j, i + 1] + (1 - xx) * yy * z[j + 1, i] + xx * yy * z[j + 1, i + 1]


class _Partner:
    """everything but `gas`: concentration 1 - C_gas(T, P), the partner of a foreign continuum"""

    def __init__(self, gas):
        self.gas, self.formula = gas, "air"

    def concentration(self, T, P):
        return 1.0 - self.gas.concentration(T, P)


class Continuum:
    """Continuum(data, gas, kind="self" | "foreign", P_ref=101325.0, T_ref=296.0, nu=None): a continuum absorber in MT_CKD form,

        sigma(nu; T, P) = x1 R(nu, T) C(nu, T) n2 / n_ref   per molecule of air,   R(nu, T) = nu tanh(c2 nu / 2T),

    held on the device as a CIA object flagged CS_CIA_RADIATION: sigma = R k Lo^2 rho1 rho2 / rhoa = R k x1 n2 with k = C / n_ref,
    n_ref = P_ref / (k_B T_ref) [molecule cm^-3].  It refreshes with the node states, runs in batches and under an
    AcceleratedAbsorber like any CIA pair.

    data: the coefficients C [cm^2 molecule^-1 per cm^-1] on a wavenumber grid -- a list of dicts {"nu", "T", "C"}, one per temperature
          (on the same samples), or a mapping {T: C-array} with the samples in `nu`.  One temperature: C does not depend on T (and the
          table is evaluated at every temperature).  Two or more: ln C is interpolated bilinearly in (nu, T); temperatures outside the
          table are refused (check_temperatures), never clamped.  Between samples ln C is linear in nu: choose the spacing accordingly.
    gas:  the absorber (molecule 1), a Gas or DirectGas of the column.
    kind: "self" pairs the gas with itself (P2 = P C_gas), "foreign" with everything else (P2 = P (1 - C_gas)).
    """

    def __init__(self, data, gas, kind: str = "self", P_ref: float = 101325.0, T_ref: float = 296.0, nu=None):
        if kind not in ("self", "foreign"):
            raise ValueError(f'kind must be "self" or "foreign", not {kind!r}')
        if not hasattr(gas, "concentration"):
            raise TypeError("gas must be a Gas or DirectGas object (the continuum's absorber)")
        if isinstance(data, dict):
            if nu is None:
                raise ValueError("a {T: C} mapping needs the wavenumber samples `nu`")
            data = [dict(nu=nu, T=T, C=C) for T, C in data.items()]
        rows = sorted(([float(d["T"]), np.asarray(d["nu"], float), np.asarray(d["C"], float)] for d in data), key=lambda r: r[0])
        if not rows:
            raise ValueError("no continuum coefficients given")
        g = rows[0][1]
        for T, v, C in rows:
            if v.shape != g.shape or not np.array_equal(v, g) or C.shape != g.shape:
                raise ValueError("every temperature must give its coefficients on the same wavenumber samples")
            if not np.all(np.isfinite(C)) or np.any(C <= 0.0):
                raise ValueError("continuum coefficients must be finite and positive (the tables hold ln C)")
        self.kind, self.gas, self.P_ref, self.T_ref = kind, gas, float(P_ref), float(T_ref)
        self.n_ref = 1e-6 * self.P_ref / (K.k * self.T_ref)                  # molecule cm^-3
        formula = getattr(gas, "formula", "X")
        self.name = f"{formula}-{formula if kind == 'self' else 'air'}"
        self.T = np.array([r[0] for r in rows])
        self.x = CIATables([dict(symbol=self.name, numin=float(g[0]), numax=float(g[-1]), npts=len(g), T=T, nu=g.copy(), k=C / self.n_ref)
                            for T, _, C in rows], extrapolate=False, singles=len(rows) == 1, radiation=True)
        self.formulae = self.x.formulae
        self.g1, self.g2 = gas, (gas if kind == "self" else _Partner(gas))

    def check_temperatures(self, T):
        """a table of two or more temperatures covers [T_min, T_max]: anything outside is an error, not a clamp"""
        if len(self.T) < 2:
            return
        T = np.atleast_1d(np.asarray(T, float))
        bad = T[(T < self.T[0]) | (T > self.T[-1])]
        if bad.size:
            raise ValueError(f"{self.kind} continuum {self.name}: temperature {bad[0]:g} K is outside the table's range "
                             f"[{self.T[0]:g}, {self.T[-1]:g}] K (extend the table: the continuum is never extrapolated)")

    def __call__(self, nu, T, P):
        """sigma(nu, T, P) [cm^2 per molecule of air], scalar nu"""
        self.check_temperatures(T)
        return cia(nu, self.x, T, P, P * self.g1.concentration(T, P), P * self.g2.concentration(T, P))

    def __repr__(self):
        return f"Continuum - {self.name} ({self.kind})"
