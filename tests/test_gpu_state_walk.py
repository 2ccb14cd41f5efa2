"""Resident columns walked across far-apart states, every absorber kind.

A column is set up once and refreshed hundreds of times in a radiative-convective run (cs_column_update_state, the re-use branch of
cs_fluxes_discretized(_members), cs_column_batch).  The other tests of that refresh move the state by a few kelvin, which selects the
same zones, live tiles and series pieces and needs the same workspace.  Here ONE column per configuration walks through states that
do not:

  A  Earth-like (workloads.earth_temperature), trace concentrations, mu 0.029
  B  hot and self-broadened: 420 K aloft to 950 K at the surface, line gas at 0.8 (+ 0.15 of the second gas), mu 0.044
  C  cold and thin: 30 .. 120 K with the top node exactly on the 25 K limit, every concentration 1e-8, mu 0.032
  A  again
  D  non-monotone: seeded uniform T in [150, 400] per level, concentrations as closures of (T, P) (as in test_column_fuzz)

on one pressure grid; P, g, grid and absorber set never change, so every step stays on the resident path (asserted: the context's
resident column is the walked one before and after each update, the column was set up exactly once, the slot count is unchanged).
The concentrations are closures of (T, P) that switch on the temperature ranges of the states, so one absorber object serves the
resident column, the fresh ones and cs_column_batch.  Baked tables and accelerated knots clip the walk to their domain.

After every step the resident column is compared with a fresh Context + Column at that state -- sigma at the nodes, tau, M+, M-
bitwise; F+, F- bitwise where two fresh columns agree bitwise (checked first), else at the suite's device-against-device 5e-13 of
the maximum -- the second visit to A with the first under the same rule, and the step with the oracle at the suite's tolerances:
1e-11 on sigma (relerr floor 1e-280; on the magnitude scale of ckdvvh_ref for the pedestal-removed codes 4 and 6) and tau, 1e-11 of
the column maximum on M and F, 2e-11 with a PHCO2 gas; every point on grids of at most 3000 points, a seeded 300-point sample
(sigma, tau, M) on longer ones.  The near-line work of Column.work() -- sub_evals + the near-zone pass + the near-line pairs of both
tiers -- must be larger at B than at A and smaller at C than at B: the walk crosses the decisions it is meant to cross.  Every
configuration carries a walked Voigt gas, which is what those counters count.

Measured on an MI355X (every case prints these under `pytest -s`).  Every comparison with a fresh column was bitwise, the band fluxes
included (two fresh columns never differed), on every grid up to 268 800 points; no residue was found.  Near-line work at A / B / C
(of which sub_evals), then the worst error against the oracle over the walk, sigma / tau / M (of the column maximum) / F:

  1 Voigt fixtures, 6000 points, interpolation on | off, main stream | side stream: 342 697 / 433 983 / 298 377 (sub 0) in all four;
      1.3e-14 / 1.1e-14 / 3.8e-13 / (sample); 2999 points, three Lobatto nodes: 550 661 / 637 790 / 509 178; 1.3e-14 / 9.8e-15 / 3.2e-12 / 6.8e-15
  2 matrix cores, 20 000 x 21: 15 488 087 / 18 954 140 / 13 281 769 (sub 0 / 497 152 / 0: only B hands cores to k_voigt_sub); 1.2e-14 / 9.7e-15 / 7.4e-14
  3 one item per wave, 92 200 x 34: 161 792 050 / 254 078 329 / 143 298 713 (sub 14 936 576 / 10 196 224 / 13 518 080); 1.0e-14 / 7.1e-15 / 5.3e-14
  4 lorentz 5541 / 7302 / 5220; 3.9e-15 / 3.5e-15 / 3.9e-14.  doppler 5541 / 7302 / 5220; 1.1e-14 / 7.4e-15 / 2.9e-14.
    PHCO2 k_phco2 10 183 / 12 275 / 9970; 1.9e-14 / 1.6e-14 / 2.2e-13.  PHCO2 k_linesum 163 213 / 163 817 / 162 633; 1.3e-14 / 1.3e-14 / 1.8e-13 / 3.5e-15.
    code 4 78 408 / 79 708 / 78 368; 1.2e-14 / 9.1e-15 / 8.4e-14 / 3.1e-15.  code 5, two groups 84 168 / 85 468 / 84 128; 1.2e-14 / 8.8e-15 / 3.2e-13 / 2.4e-15.
    code 6 78 408 / 79 708 / 78 368; 1.2e-14 / 9.2e-15 / 2.6e-13 / 3.5e-15.  shifted voigt 276 133 / 298 944 / 263 376; 1.4e-14 / 1.2e-14 / 7.1e-13 / 4.7e-15;
    shifted lorentz and doppler 4901 / 6272 / 4496; 7.4e-15 / 6.9e-15 / 1.7e-12 / 2.8e-15 and 1.4e-14 / 1.0e-14 / 2.4e-13 / 2.2e-15
  5 baked beside direct (walk clipped to 160 .. 480 K) 5541 / 6311 / 5485; 6.4e-14 / 5.4e-14 / 1.0e-13.  CIA pairs 343 099 / 439 089 / 298 450;
    1.3e-14 / 8.7e-15 / 3.5e-13.  gray + beam + albedo 291 408 / 337 260 / 269 167; 1.0e-14 / 8.9e-15 / 8.8e-13 / 2.8e-15.  accelerated knots: sigma 1.7e-14
  6 mixed precision 1 258 309 / 1 365 424 / 1 207 323; against fp64: sigma 4.2e-7, OLR 4.2e-8 W/m^2
  7 flux forms, 300 / 600 / 2000 / 4200 tiles: 458 310 / 662 059 / 355 670; 687 037 / 1 082 474 / 484 722; 1 731 814 / 3 065 501 / 1 068 313;
    3 379 860 / 6 176 255 / 1 984 247 (the same under key 15 = 1); sigma 1.2e-14, tau 9.3e-15, M 2.8e-12
  8 host-pointer entry: tau 9.9e-15 (6.9e-14 with the baked table), M 5.1e-13 (4.4e-12), F 2.4e-15 (6.2e-15)
  9 batch after the walk: 550 661 / 637 790 / 509 178; batch against sequential 2.5e-16
"""
import os

import numpy as np
import pytest

import ckdvvh_ref as X
import voigt_lbl_ref as V
import workloads as W
from conftest import HITRAN, relerr

pytestmark = pytest.mark.gpu

G = 9.8
ORDER = "ABCAD"
MU = dict(A=0.029, B=0.044, C=0.032, D=0.029)


# ---- the states -----------------------------------------------------------------------------------------------------------------

def fC1(T, P):
    """the line gas: 0.8 in state B (T >= 420 K), 1e-8 in state C (T <= 120 K), a trace that grows with pressure in between"""
    return 0.8 if T > 405.0 else (1e-8 if T < 125.0 else 4e-4 * (1.0 + P / 1e5))


def fC2(T, P):
    """the second gas: 0.15 in B, 1e-8 in C, test_column_fuzz's closure of (T, P) in between"""
    return 0.15 if T > 405.0 else (1e-8 if T < 125.0 else min(0.05, 1e-3 * (P / 1e5) ** 2 * (T / 250.0) ** 4))


def states(P, Tlim=(25.0, 1000.0)):
    """level temperatures of A, B, C, D on the pressure grid P, clipped to Tlim (a baked domain, the accelerated knots)"""
    x = np.log(P / P[0]) / np.log(P[-1] / P[0])            # 0 at the top, 1 at the surface
    T = dict(A=W.earth_temperature(P), B=420.0 + 530.0 * x, C=30.0 + 90.0 * x,
             D=np.random.default_rng(20261017).uniform(150.0, 400.0, len(P)))
    T["C"][0] = 25.0                                       # the limit of the Qref/Q fits, touched at the top node
    return {k: np.clip(v, *Tlim) for k, v in T.items()}


# ---- one column, its outputs, its reference ---------------------------------------------------------------------------------------

class Spec:
    """one configuration: grid, levels, rule orders, context settings, absorbers"""

    def __init__(self, nu, npl, members, tune=(), core=(5, 2), fS=0.0, fa=0.0, Pt=10.0, Tlim=(25.0, 1000.0), order=ORDER, tol=1e-11,
                 form=None, setup=None, cia_data=None, check=None, oracle=True):
        self.nu, self.P, self.members, self.tune, self.core = nu, None, members, tune, core
        self.npl, self.Pt, self.fS, self.fa, self.Tlim, self.order, self.tol, self.form = npl, Pt, fS, fa, Tlim, order, tol, form
        self.setup, self.cia_data, self.check, self.oracle = setup, cia_data or {}, check, oracle

    def context(self, cs):
        ctx = cs.Context(0)
        if self.setup is not None:
            self.setup(ctx)
        for k, v in self.tune:
            ctx.set_tuning(k, v)
        return ctx

    def column(self, cs, ctx, T, mu):
        P = cs.pressuregrid(self.Pt, 1e5, self.npl)
        return cs.Column(P, G, T, mu, self.fS, self.fa, *self.members(cs, ctx, self.nu), core=cs.Discretized(*self.core), ctx=ctx,
                         _warn=False)


def outputs(col):
    col.run()
    tau = np.zeros((col.nl, col.nnu), order="F")
    Mu = np.zeros((col.np, col.nnu), order="F")
    Md = np.zeros((col.np, col.nnu), order="F")
    Fup, Fdn = col.fetch(tau, Mu, Md)
    w, info = col.work(), col.info()
    return dict(tau=tau, Mup=Mu, Mdn=Md, Fup=Fup, Fdn=Fdn, work=w, info=info, sigma=col.sigma_nodes())


def near_work(w):
    return w["sub_evals"] + w["direct_by_body"]["near_zone"] + w["near_pairs_tier0"] + w["near_pairs_tier1"]


def fresh(cs, spec, T, mu):
    ctx = spec.context(cs)
    try:
        return outputs(spec.column(cs, ctx, T, mu))
    finally:
        ctx.close()


def special_sigma(cs, O, spec, col, gi, x):
    """(C_k sigma, C_k magnitude) [K, len(x)] of a column gas the oracle has no shape for, from the suite's restatements"""
    g = col.gases[gi]
    code = cs.SHAPES[g.shape]
    val, mag = np.zeros((col.K, len(x))), np.zeros((col.K, len(x)))
    for k in range(col.K):
        Ck, Tk, Pk = col.conc[gi, k], col.Tk[k], col.Pk[k]
        if g.pressure_shift:
            import test_gpu_pressure_shift as PS
            v = PS.expected(O, g.sl, g.sl.delta_a, g.shape, x, Tk, Pk, Ck * Pk, False, g.dnu_cut)
            m = v
        elif code == 7:
            v, m = V.expected(cs, O, g.sl, g.sl.delta_a, x, Tk, Pk, Ck * Pk, g.dnu_cut, False)
        else:
            v, m = X.expected(cs, O, g.sl, x, Tk, Pk, Ck * Pk, g.dnu_cut, strict=False, ped=code in (4, 6), vvh=code in (5, 6))
        val[k], mag[k] = Ck * v, Ck * np.abs(m)
    return val, mag


def reference(cs, O, spec, col, idx):
    """the oracle column at the points idx: its own four shapes natively, everything else as sigma_extra from the suite's restatements.
    Returns the oracle's dict and the scale sigma is measured against (the values themselves but for the pedestal-removed codes)."""
    x = col.nu[idx]
    native = [gi for gi, g in enumerate(col.gases) if cs.SHAPES[g.shape] < 4 and not g.pressure_shift]
    extra, mag = np.zeros((col.K, len(x))), np.zeros((col.K, len(x)))
    for gi in range(len(col.gases)):
        if gi not in native:
            v, m = special_sigma(cs, O, spec, col, gi, x)
            extra += v
            mag += m
    for ti, g in enumerate(col.baked):
        for k in range(col.K):
            v = col.conc_tab[ti, k] * O.table_sigma(g.lnsigma[idx], g.Omega.T, g.Omega.P, col.Tk[k], col.Pk[k])
            extra[k] += v
            mag[k] += v
    for ci, c in enumerate(col.U.cia):
        for k in range(col.K):
            v = O.cia_sigma(spec.cia_data[c.name], x, col.Tk[k], col.Pk[k], col.cia_P1[ci, k], col.cia_P2[ci, k], c.x.extrapolate, c.x.singles)
            extra[k] += v
            mag[k] += v
    if col.sigma_extra is not None:
        extra += col.sigma_extra[:, idx]
        mag += col.sigma_extra[:, idx]
    conc = col.conc[native] if native else np.zeros((0, col.K))
    r = O.fluxes_discretized(x, col.P, col.g, col.core.nlobatto, col.Tn, col.mun, col.Tlev, [col.gases[gi].sl for gi in native],
                             [col.gases[gi].shape for gi in native], [col.gases[gi].dnu_cut for gi in native], conc,
                             sigma_gray=col.sigma_gray, sigma_extra=extra, S_toa=None if col.S_toa is None else col.S_toa[idx],
                             albedo=None if col.albedo is None else col.albedo[idx], theta_s=col.theta_s, nstream=col.core.nstream,
                             want_sigma=True)
    return r, (r["sigma"] - extra) + mag


def sample(n):
    return np.arange(n) if n <= 3000 else np.sort(np.random.default_rng(n).choice(n, 300, replace=False))


def vs_oracle(cs, O, spec, col, r, worst, reference=reference):
    n = col.nnu
    idx = sample(n)
    ref, scale = reference(cs, O, spec, col, idx)
    sm = max(ref["Mup"].max(), ref["Mdn"].max())
    e = dict(sigma=float(np.max(np.abs(r["sigma"][:, idx] - ref["sigma"]) / np.maximum(scale, 1e-280))),
             tau=relerr(r["tau"][:, idx], ref["tau"]),
             Mup=float(np.max(np.abs(r["Mup"][:, idx] - ref["Mup"])) / sm), Mdn=float(np.max(np.abs(r["Mdn"][:, idx] - ref["Mdn"])) / sm))
    if len(idx) == n:
        fm = max(np.abs(ref["Fup"]).max(), np.abs(ref["Fdn"]).max())
        e["Fup"], e["Fdn"] = float(np.max(np.abs(r["Fup"] - ref["Fup"])) / fm), float(np.max(np.abs(r["Fdn"] - ref["Fdn"])) / fm)
    for k, v in e.items():
        worst[k] = max(worst.get(k, 0.0), v)
    return e


def same_as(r, f, flux_bitwise, label):
    """the resident column's outputs against another evaluation of the same state: bitwise; the band fluxes at 5e-13 of the maximum
    where two fresh columns were seen to differ bitwise (band partials added with device-scope atomics on long grids)"""
    for k in ("sigma", "tau", "Mup", "Mdn"):
        assert np.array_equal(r[k], f[k]), (label, k, float(np.nanmax(np.abs(r[k] - f[k]))), np.argwhere(r[k] != f[k])[:4].tolist())
    fm = max(np.abs(f["Fup"]).max(), np.abs(f["Fdn"]).max())
    for k in ("Fup", "Fdn"):
        if flux_bitwise:
            assert np.array_equal(r[k], f[k]), (label, k, float(np.max(np.abs(r[k] - f[k])) / fm))
        else:
            assert np.max(np.abs(r[k] - f[k])) < 5e-13 * fm, (label, k, float(np.max(np.abs(r[k] - f[k])) / fm))


def walk(cs, O, spec, name, keep=False):
    """the walk of one configuration; returns (context, column, per-state outputs) with keep (the caller closes the context)"""
    T = states(cs.pressuregrid(spec.Pt, 1e5, spec.npl), spec.Tlim)
    ctx = spec.context(cs)
    try:
        col = spec.column(cs, ctx, T[spec.order[0]], MU[spec.order[0]])
        setups, inner = [0], col._setup

        def counted():
            setups[0] += 1
            inner()
        col._setup = counted
        nslots = len(ctx._slots)
        seen, near, worst, bitwise = {}, {}, {}, {}
        for step, s in enumerate(spec.order):
            if step:
                assert ctx._resident is col
                col.update(T[s], MU[s])
            r = outputs(col)
            assert ctx._resident is col and setups[0] == 0 and len(ctx._slots) == nslots, (name, step, s, setups[0])
            if spec.form is not None:
                assert r["info"]["flux_form"] == spec.form, (name, s, r["info"])
            if s in seen:
                same_as(r, seen[s], bitwise[s], f"{name}: second visit to {s}")
            else:
                f1, f2 = fresh(cs, spec, T[s], MU[s]), fresh(cs, spec, T[s], MU[s])
                bitwise[s] = bool(np.array_equal(f1["Fup"], f2["Fup"]) and np.array_equal(f1["Fdn"], f2["Fdn"]))
                for k in ("sigma", "tau", "Mup", "Mdn"):
                    assert np.array_equal(f1[k], f2[k]), (name, s, k, "two fresh columns differ")
                same_as(r, f1, bitwise[s], f"{name}: step {step} ({s}) against a fresh column")
                e = vs_oracle(cs, O, spec, col, r, worst) if spec.oracle else {}
                near[s] = near_work(r["work"])
                print(f"  {name} {s}: near-line work {near[s]} (sub {r['work']['sub_evals']}, zone {r['work']['direct_by_body']['near_zone']}, "
                      f"pairs {r['work']['near_pairs_tier0']} + {r['work']['near_pairs_tier1']}), form {r['info']['flux_form']}, F bitwise "
                      f"{bitwise[s]}, oracle " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
                seen[s] = r
        print(f"  {name}: worst oracle error " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
        assert near["B"] > near["A"] and near["C"] < near["B"], (name, near)
        for k, v in worst.items():
            assert v < spec.tol, (name, k, v)
        if spec.check is not None:
            spec.check(cs, spec, seen, T)
        if keep:
            return ctx, col, seen, T
    finally:
        if not keep:
            ctx.close()


# ---- absorber sets ----------------------------------------------------------------------------------------------------------------

def fixtures(shape1="voigt", shape2="voigt", **kw):
    def members(cs, ctx, nu):
        return [cs.DirectGas(W.lines("fixture", "CO2"), fC1, nu, shape=shape1, **kw), cs.DirectGas(W.lines("fixture", "H2O"), fC2, nu, shape=shape2)]
    return members


NU_A = np.linspace(640.0, 700.0, 6000)                      # 94 tiles: the plane-residue grid
NU_S = np.linspace(640.0, 700.0, 2999)                      # every point against the oracle, band fluxes included


def interp_off(ctx):
    ctx.set_interp(False)


def _near_stream(on):
    def check(cs, spec, seen, T):
        for s, r in seen.items():      # cs_column_work out[37], bit 2: the near-line kernels on their side stream, adding into their own plane
            assert bool(r["work"]["dispatch"]["streams"] & 2) == on, (s, r["work"]["dispatch"])
    return check


VOIGT = {
    "interp-on": Spec(NU_A, 9, fixtures(), check=_near_stream(False)),
    "interp-off": Spec(NU_A, 9, fixtures(), setup=interp_off, check=_near_stream(False)),
    "interp-on-side-stream": Spec(NU_A, 9, fixtures(), tune=((7, 2),), check=_near_stream(True)),
    "interp-off-side-stream": Spec(NU_A, 9, fixtures(), tune=((7, 2),), setup=interp_off, check=_near_stream(True)),
    "whole-grid": Spec(NU_S, 9, fixtures(), core=(4, 3)),
}


@pytest.mark.parametrize("name", list(VOIGT))
def test_voigt_merged_fixtures(cs, O, name):
    """configuration 1: H2O + CO2 fixtures merged into one launch group, interpolation on and off, the near-line kernels on the main
    stream (default on this grid) and on their side stream with a plane of their own (key 7 = 2); and once on a grid short enough
    for every point and the band fluxes to meet the oracle, with three Lobatto nodes"""
    walk(cs, O, VOIGT[name], name)


def synthetic(shape="voigt"):
    def members(cs, ctx, nu):
        return [cs.DirectGas(W.lines("synthetic", "CO2"), fC1, nu, shape=shape), cs.DirectGas(W.lines("synthetic", "H2O"), fC2, nu)]
    return members


def matrix_cores(ctx):
    ctx.set_matrix_cores(2)


def _pieces_move(cs, spec, seen, T):
    """the hot, self-broadened state has other series radii: lines move between the matrix-core pieces and the vector unit, and some
    window cores go to the sub-tile kernel, which no tile of states A and C needs"""
    a, b, c = (seen[s]["work"] for s in "ABC")
    assert a["node_evals_matrix"] > 0 and a["direct_evals_matrix"] > 0, a
    assert b["node_evals_matrix"] != a["node_evals_matrix"] and b["matrix_evals_3term"] != a["matrix_evals_3term"], (a, b)
    assert b["sub_evals"] > 0 and a["sub_evals"] == 0 and c["sub_evals"] == 0, (a["sub_evals"], b["sub_evals"], c["sub_evals"])


def test_matrix_core_forms(cs, O):
    """configuration 2: the synthetic bench tables on 20 000 points at 0.01 cm^-1, 21 levels, the matrix-core kernels forced on"""
    walk(cs, O, Spec(600.0 + 0.01 * np.arange(20000), 21, synthetic(), setup=matrix_cores, check=_pieces_move), "matrix-cores")


def _one_item_per_wave(cs, spec, seen, T):
    for s in "ABC":
        w = seen[s]["work"]
        assert w["edge_mx_flops_useful"] > 0 and w["node_evals_matrix"] > 0 and w["sub_evals"] > 0, (s, w)


def test_one_item_per_wave_forms(cs, O):
    """configuration 3: 1441 tiles and 720 smallest intervals with K = 34 (three state groups): k_voigt_edge_mx and k_cheb_nodes_mx take
    one (tile | interval, group) per wave (mx_big), as in test_interp_fuzz_long; three states, the oracle on the sample"""
    spec = Spec(100.0 + 0.025 * np.arange(92200), 34, synthetic(), setup=matrix_cores, order="ABC", check=_one_item_per_wave)
    assert (len(spec.nu) + 63) // 64 * 3 >= 1024 and len(spec.nu) // 128 * 3 >= 2048
    walk(cs, O, spec, "one-item-per-wave")


# ---- every shape code -------------------------------------------------------------------------------------------------------------------

def h2o_low(cs):
    if "low" not in _tables:
        _tables["low"] = cs.SpectralLines(os.path.join(HITRAN, "H2O.par"), numin=0.0, numax=150.0)
    return _tables["low"]


def dense(cs):
    if "dense" not in _tables:
        _tables["dense"] = cs.SpectralLines.synthetic(2, 8000, 91, numin=200.0, numax=1400.0)
    return _tables["dense"]


_tables = {}


def phco2(table):
    def members(cs, ctx, nu):
        sl = dense(cs) if table == "dense" else W.lines("fixture", "CO2")
        return [cs.DirectGas(sl, fC1, nu, shape="PHCO2"), cs.DirectGas(W.lines("fixture", "H2O"), fC2, nu)]
    return members


def low(shape, second_cut=None):
    """the H2O lines below 150 cm^-1 under `shape` on a grid from 0.5 cm^-1 (mirror terms in the first 25), optionally CO2 under the
    same shape with another cut-off (a second launch group of that code), and the same H2O lines once more as the walked Voigt gas"""
    def members(cs, ctx, nu):
        m = [cs.DirectGas(h2o_low(cs), fC2, nu, shape=shape)]
        if second_cut is not None:
            m.append(cs.DirectGas(W.lines("fixture", "CO2"), fC1, nu, shape=shape, dnu_cut=second_cut))
        return m + [cs.DirectGas(h2o_low(cs), fC1, nu)]
    return members


def _line_kernel(which):
    def check(cs, spec, seen, T):
        for s, r in seen.items():
            assert r["info"]["line_kernel"] == which, (s, r["info"])
    return check


def _two_groups_of(n):
    def check(cs, spec, seen, T):
        assert seen["A"]["info"]["groups"] == n, seen["A"]["info"]
    return check


NU_P = np.linspace(640.0, 800.0, 6401)                      # test_phco2_interpolated_wings' grid: k_phco2 with interpolated wings
NU_G = np.linspace(100.0, 1300.0, 2400)                     # tiles wider than a chi-region: PHCO2 through k_linesum
NU_L = np.linspace(0.5, 120.0, 2990)
SHAPES = {
    "lorentz": Spec(NU_A, 9, fixtures("lorentz")),
    "doppler": Spec(NU_A, 9, fixtures("doppler")),
    "phco2-fast": Spec(NU_P, 9, phco2("dense"), tol=2e-11),
    "phco2-generic": Spec(NU_G, 9, phco2("fixture"), tol=2e-11),
    "code4": Spec(NU_L, 9, low("voigtCKD")),
    "code5-two-groups": Spec(NU_L, 9, low("voigtVVH", 20.0), check=_two_groups_of(3)),
    "code6": Spec(NU_L, 9, low("voigtCKDVVH")),
    # pressure shifts with arbitrary delta and P: 1e-9 (test_gpu_pressure_shift's docstring: the device rounds nul + s, the oracle nu - s)
    "voigt-shifted": Spec(NU_S, 9, fixtures("voigt", pressure_shift=True), tol=1e-9),
    "lorentz-shifted": Spec(NU_S, 9, fixtures("lorentz", pressure_shift=True), tol=1e-9),
    "doppler-shifted": Spec(NU_S, 9, fixtures("doppler", pressure_shift=True), tol=1e-9),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_shape_code(cs, O, name):
    """configuration 4: each shape code through the column beside a walked Voigt gas; expected values of codes 4 - 6 from ckdvvh_ref,
    of the shifted codes from test_gpu_pressure_shift.expected"""
    walk(cs, O, SHAPES[name], name)


# ---- other members ------------------------------------------------------------------------------------------------------------------------

DOMAIN = (150.0, 500.0)


def baked(cs, ctx, nu):
    Om = cs.AtmosphericDomain(DOMAIN, 8, (5.0, 2e5), 10)
    g = cs.Gas(W.lines("fixture", "CO2"), lambda T, P: min(0.3, 1e-3 * (P / 1e5) * (T / 250.0) ** 4), nu, Om, ctx=ctx, keep_host_tables=True)
    return [g, cs.DirectGas(W.lines("fixture", "H2O"), fC2, nu)]


def _cia_sets():
    import tabulated_ref as R
    a = R.band(630.0, 671.3, 40, R.TS, 1) + R.band(655.1, 710.0, 7, R.TS[:3], 2)
    b = R.band(600.0, 720.0, 33, R.TS[1:], 3, symbol="CO2-CH4")
    return {"CO2-CO2": a, "CO2-CH4": b}


def cia_pairs(cs, ctx, nu):
    d = _cia_sets()
    return [cs.DirectGas(W.lines("fixture", "CO2"), fC1, nu), cs.DirectGas(W.lines("fixture", "CH4"), fC2, nu),
            cs.CIATables(d["CO2-CO2"], extrapolate=True), cs.CIATables(d["CO2-CH4"])]


def gray_beam(cs, ctx, nu):
    return fixtures()(cs, ctx, nu) + [cs.GrayGas(2e-26, nu)]


MEMBERS = {
    "baked-beside-direct": Spec(NU_A, 9, baked, Tlim=(160.0, 480.0)),
    "cia-pairs": Spec(NU_A, 9, cia_pairs, cia_data=_cia_sets()),
    "gray-beam-albedo": Spec(NU_S, 9, gray_beam, fS=lambda v: 2e-3 * np.exp(-((v - 670.0) / 20.0) ** 2), fa=0.3),
}


@pytest.mark.parametrize("name", list(MEMBERS))
def test_other_members(cs, O, name):
    """configuration 5: a baked Gas beside a direct gas (the walk clipped to the table's domain), both CIA pairs on synthetic bands
    (states in and out of the bands' temperature ranges, one pair extrapolating), the gray term with a stellar beam and an albedo"""
    walk(cs, O, MEMBERS[name], name)


def test_accelerated_knots(cs, O):
    """configuration 5, the AcceleratedAbsorber: update_ walked through the same temperatures; cs_accel_fetch bitwise against a fresh
    AcceleratedAbsorber on a fresh context, at 1e-14 of max |ln sigma| against ln of a fresh knot column's cross-sections
    (test_batch_accel_shards' bound) and at 1e-11 in sigma against the oracle at the knots"""
    nu = NU_S
    Pk = cs.pressuregrid(10.0, 1e5, 12)
    T = states(Pk)

    def knots(ctx, A):
        kn = np.zeros((len(Pk), len(nu)))
        cs.check(cs.lib().cs_accel_fetch(ctx.handle, A.slot, len(nu), len(Pk), cs.dptr(kn)))
        return kn
    ctx = cs.Context(0)
    try:
        A = cs.AcceleratedAbsorber(T["A"], Pk, *fixtures()(cs, ctx, nu), ctx=ctx)
        first = {}
        for step, s in enumerate(ORDER):
            if step:
                A.update_(T[s])
            assert ctx._resident is A._knots
            kn = knots(ctx, A)
            if s in first:
                assert np.array_equal(kn, first[s])
                continue
            first[s] = kn
            c2 = cs.Context(0)
            try:
                B = cs.AcceleratedAbsorber(T[s], Pk, *fixtures()(cs, c2, nu), ctx=c2)
                assert np.array_equal(kn, knots(c2, B)), s
                B._knots.sigma_run()
                sig = B._knots.sigma_nodes()
                kc = B._knots
                del B
            finally:
                c2.close()
            assert not np.any(np.isnan(kn)) and np.max(np.abs(kn - np.log(sig))) < 1e-14 * np.max(np.abs(np.log(sig))), s
            r = O.fluxes_discretized(nu, Pk, 1.0, 2, kc.Tn, kc.mun, kc.Tlev, [g.sl for g in kc.gases], ["voigt"] * 2, [25.0] * 2, kc.conc,
                                     nstream=1, want_sigma=True)
            e = relerr(np.exp(kn), r["sigma"], floor=1e-280)
            print(f"  accelerated knots {s}: sigma against the oracle {e:.1e}")
            assert e < 1e-11, (s, e)
    finally:
        ctx.close()


# ---- mixed precision -------------------------------------------------------------------------------------------------------------------------

def _mixed(ctx):
    ctx.set_precision("mixed", 1e6)


def _against_fp64(cs, spec, seen, T):
    """test_mixed_precision_variant's bounds: cross-sections within 1e-6 of the fp64 path, OLR within 1e-5 W/m^2"""
    ref = Spec(spec.nu, spec.npl, spec.members, core=spec.core)
    for s in "ABCD":
        f = fresh(cs, ref, T[s], MU[s])
        m = f["sigma"] > 0
        e = float(np.max(np.abs(seen[s]["sigma"][m] / f["sigma"][m] - 1.0)))
        print(f"  mixed {s}: sigma against fp64 {e:.1e}, OLR {abs(seen[s]['Fup'][0] - f['Fup'][0]):.1e} W/m^2")
        assert e < 1e-6 and abs(seen[s]["Fup"][0] - f["Fup"][0]) < 1e-5, (s, e)
    assert not np.array_equal(seen["A"]["sigma"], fresh(cs, ref, T["A"], MU["A"])["sigma"])      # (the fp32 bodies really ran)


def test_mixed_precision(cs, O):
    """configuration 6: fp32 far wings (far_s = 1e6): resident against fresh bitwise, against fp64 at test_mixed_precision_variant's bounds"""
    walk(cs, O, Spec(np.linspace(600.0, 760.0, 4000), 21, fixtures(), setup=_mixed, oracle=False, check=_against_fp64), "mixed")


# ---- flux forms ------------------------------------------------------------------------------------------------------------------------------

def _forms():
    from test_gpu_voigt_vvh import FORMS
    return FORMS


@pytest.mark.parametrize("tiles,tune,form,streams", _forms(), ids=[f"{t}tiles-{f}{'-streams' if s else ''}{'-unfused' if u else ''}"
                                                                 for t, u, f, s in _forms()])
def test_flux_forms(cs, O, tiles, tune, form, streams):
    """configuration 7: the walk under every flux form the step dispatches (test_gpu_voigt_vvh.FORMS: grid size and key 15), a plain
    Voigt gas; the form is asserted at every step"""
    def one(cs, ctx, nu):
        return [cs.DirectGas(W.lines("fixture", "CO2"), fC1, nu)]

    def flags(cs, spec, seen, T):
        for s, r in seen.items():
            assert bool(r["work"]["dispatch"]["flags"] & 4) == streams, (s, r["work"]["dispatch"])
    walk(cs, O, Spec(np.linspace(640.0, 700.0, 64 * tiles), 9, one, tune=tuple(tune.items()), form=form, check=flags), f"{tiles} tiles, form {form}")


# ---- the host-pointer entry --------------------------------------------------------------------------------------------------------------------

def _host_call(cs, spec, ctx, T, mu, extra, beam, albedo):
    """one call of cs_fluxes_discretized(_members) through ctypes (core._fluxes_discretized marshals as the Julia ccall does): NULL or an
    array for sigma_extra, S_toa and albedo"""
    P = cs.pressuregrid(spec.Pt, 1e5, spec.npl)
    m = spec.members(cs, ctx, spec.nu)
    if extra:
        m = m + [lambda v, T_, P_: 3e-27 * (P_ / 1e5) * (T_ / 250.0) * np.ones_like(v)]
    d = cs.Column(P, G, T, mu, (lambda v: 2e-3 * np.exp(-((v - 670.0) / 20.0) ** 2)) if beam else None, 0.3 if albedo else None, *m,
                  core=cs.Discretized(*spec.core), ctx=ctx, _setup=False, _warn=False)
    tau = np.zeros((d.nl, d.nnu), order="F")
    Mu = np.zeros((d.np, d.nnu), order="F")
    Md = np.zeros((d.np, d.nnu), order="F")
    Fup, Fdn = cs.core._fluxes_discretized(d, tau, Mu, Md)
    return d, dict(tau=tau, Mup=Mu, Mdn=Md, Fup=Fup, Fdn=Fdn)


# NULL / array per call: every transition (0 -> 1, 1 -> 1, 1 -> 0, 0 -> 0) of each of the three pointers over the five calls
TOGGLE = dict(extra=(0, 1, 1, 0, 0), beam=(1, 1, 0, 0, 1), albedo=(1, 0, 0, 1, 1))


@pytest.mark.parametrize("name", ["cs_fluxes_discretized", "cs_fluxes_discretized_members"])
def test_host_pointer_entry(cs, O, name):
    """configuration 8: the same walk through the host-pointer symbols, whose re-use branch keeps the resident column when only the
    state and the per-call spectra change; sigma_extra, S_toa and albedo toggle between NULL and an array through every transition.
    Each call against the same call on a fresh context (tau, M+, M- bitwise, F under the rule of the walk) and against the oracle"""
    spec = Spec(NU_S, 9, fixtures()) if name == "cs_fluxes_discretized" else Spec(NU_S, 9, baked, Tlim=(160.0, 480.0))
    T = states(cs.pressuregrid(spec.Pt, 1e5, spec.npl), spec.Tlim)
    ctx = spec.context(cs)
    worst = {}
    try:
        members = spec.members(cs, ctx, spec.nu)            # (one set of absorbers for the walked context: a baked table is baked once)
        walked = Spec(spec.nu, spec.npl, lambda *_: list(members), Tlim=spec.Tlim)
        for step, s in enumerate(ORDER):
            tg = {k: bool(v[step]) for k, v in TOGGLE.items()}
            d, r = _host_call(cs, walked, ctx, T[s], MU[s], **tg)
            assert (d.sigma_extra is not None) == tg["extra"] and (d.S_toa is not None) == tg["beam"] and (d.albedo is not None) == tg["albedo"]
            fr = []
            for _ in range(2):
                c2 = spec.context(cs)
                try:
                    fr.append(_host_call(cs, spec, c2, T[s], MU[s], **tg)[1])
                finally:
                    c2.close()
            bitwise = bool(np.array_equal(fr[0]["Fup"], fr[1]["Fup"]) and np.array_equal(fr[0]["Fdn"], fr[1]["Fdn"]))
            fm = max(np.abs(fr[0]["Fup"]).max(), np.abs(fr[0]["Fdn"]).max())
            for k in ("tau", "Mup", "Mdn", "Fup", "Fdn"):
                if k[0] != "F" or bitwise:
                    assert np.array_equal(r[k], fr[0][k]), (name, step, s, tg, k, float(np.max(np.abs(r[k] - fr[0][k]))))
                else:
                    assert np.max(np.abs(r[k] - fr[0][k])) < 5e-13 * fm, (name, step, s, tg, k)
            ref, _ = reference(cs, O, walked, d, np.arange(d.nnu))
            sm = max(ref["Mup"].max(), ref["Mdn"].max(), 1e-300)
            fmr = max(np.abs(ref["Fup"]).max(), np.abs(ref["Fdn"]).max())
            e = dict(tau=relerr(r["tau"], ref["tau"]), Mup=float(np.max(np.abs(r["Mup"] - ref["Mup"])) / sm),
                     Mdn=float(np.max(np.abs(r["Mdn"] - ref["Mdn"])) / sm), Fup=float(np.max(np.abs(r["Fup"] - ref["Fup"])) / fmr),
                     Fdn=float(np.max(np.abs(r["Fdn"] - ref["Fdn"])) / fmr))
            print(f"  {name} call {step} ({s}, {tg}): F bitwise {bitwise}, oracle " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
                assert v < 1e-11, (name, step, s, k, v)
    finally:
        ctx.close()


# ---- a batch after the walk -----------------------------------------------------------------------------------------------------------------------

def test_batch_after_walk(cs, O):
    """configuration 9: cs_column_batch of the five states on the column that has just been walked, against the five sequential
    results at test_batched_columns_match_sequential's bound, 1e-13 of the largest upward flux"""
    ctx, col, seen, T = walk(cs, O, Spec(NU_S, 9, fixtures(), core=(5, 3)), "batch", keep=True)
    try:
        Fu, Fd = col.run_batch([T[s] for s in ORDER], [MU[s] for s in ORDER])
        assert ctx._resident is col
        for b, s in enumerate(ORDER):
            a = seen[s]
            e = max(np.max(np.abs(Fu[b] - a["Fup"])), np.max(np.abs(Fd[b] - a["Fdn"]))) / a["Fup"].max()
            print(f"  batch profile {b} ({s}): {e:.1e}")
            assert e < 1e-13, (b, s, e)
    finally:
        ctx.close()
