"""The two reduced outputs of a resident column -- want_M="edges" (M+, M- at level 0 and level np-1, [2, nnu]) and want_M="tiles" (sum of
w_j M[level, j] over every 64-point tile, [np, ntile]) -- against the planes of a want_M=True column, in every flux kernel form.

All forms store through one helper (level_out, cs_kernels.h), so a case = (form, NS, grid, levels, Lobatto order) runs THREE columns with
the same cs_set_tuning keys -- planes, edges, tiles -- and asserts of each the form it reports (Column.info()["flux_form"]: 0 separate
kernels, 2 chunk, 3 scan; Column.work()["dispatch"]["flags"]: RT_STREAMS, CHUNK4), so that the columns of a comparison ran the same
instance.  Fixtures, members (CO2 line by line, a gray term, a stellar beam, an albedo function, a CIA pair in part of the cases) and the
keys that force each form are tests/test_gpu_flux_orders.py's:

  k_rt<NS, true>      key 15 = 1, key 5 = 0        NS 4, 10
  k_rt_streams<NS>    key 15 = 1                   NS 4
  k_flux_scan<NS, 5>  default keys                 NS 4
  k_flux_scan<NS, 0>  key 15 = 2048                NS 4
  k_flux_chunk3<NS>   key 15 = 2, key 5 = 0        NS 4, 10
  k_flux_chunk<NS>    key 15 = 2 | 8, key 5 = 0    NS 4, 10

Grids: 2577 points (41 tiles, a last tile of 17 points), 17, 64 and 65 points; np = 2 (both edges are all there is) and np = 9; nlobatto 2
and 3 -- (np, nlobatto) rotates over the cases of a form so that every form meets both values of each.

Bounds.  Edge spectra and band fluxes: bitwise (the mode changes what is stored, not what is computed).  A tile sum against
math.fsum(w_j M[i, j]) of the planes column: 66 x 2^-53 x sum_j |w_j M_j| -- one rounding per product and 63 additions in whatever order
the wave reduction takes; all terms are non-negative.  fsum over the tiles of a level against its band flux: (ntile + 66) x 2^-53 x F.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import clearsky_jl_amd
import workloads as W
import test_gpu_flux_orders as FO
from test_gpu_boundary import _julia_call
from conftest import source_rounding_bound

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CS_ESTATE = -6
SENTINEL = -7.25e300                             # (no flux is negative)
_dp = C.POINTER(C.c_double)

# form name -> (cs_set_tuning keys, flux_form, RT_STREAMS flag, CHUNK4 flag, stream counts)
FORMS = {
    "rt_ud": (((15, 1), (5, 0)), 0, False, False, (4, 10)),
    "rt_streams": (((15, 1),), 0, True, False, (4,)),
    "scan5": ((), 3, False, False, (4,)),
    "scan0": (((15, 2048),), 3, False, False, (4,)),
    "chunk3": (((15, 2), (5, 0)), 2, False, False, (4, 10)),
    "chunk": (((15, 2 | 8), (5, 0)), 2, False, True, (4, 10)),
}
GRIDS = (FO.N_SHORT, 17, 64, 65)
SHAPES = ((2, 2), (9, 3), (9, 2), (2, 3))        # (np, nlobatto)


def _cases():
    out = []
    for form, (_, _, _, _, nss) in FORMS.items():
        q = 0
        for ns in nss:
            for n in GRIDS:
                np_, nlob = SHAPES[q % 4]
                cia = n == FO.N_SHORT and form in ("scan5", "chunk3", "rt_ud") and ns == 4      # a CIA pair: the fused forms add it per tile / per 16-state load
                out.append(pytest.param(form, ns, n, np_, nlob, cia, id=f"{form}-ns{ns}-n{n}-np{np_}-lob{nlob}" + ("-cia" if cia else "")))
                q += 1
            q += 1                                # (the second stream count meets the grids with the other shapes)
    return out


def _column(ns, nlob, n, np_, ctx, cia=False, **kw):
    """test_gpu_flux_orders._column, which also takes np = 2: one layer from 5 Pa to the surface (pressuregrid starts at three levels)"""
    cs = clearsky_jl_amd
    if np_ > 2:
        return FO._column(ns, nlob, n, np_, ctx, cia, **kw)
    P = np.array([5.0, 1e5])
    return cs.Column(P, 9.8, W.earth_temperature(P), 0.029, FO.FS, FO.FA, *FO._members(FO._nu(n), cia), core=cs.Discretized(ns, nlob),
                     theta_s=FO.THETA_S, ctx=ctx, _warn=False, **kw)


def _one(form, ns, n, np_, nlob, cia, want_M, nu_range=None, tune=None):
    """one column in the given mode under the form's keys: what it returns, the form it reports"""
    cs = clearsky_jl_amd
    keys, flux_form, streams, chunk4, _ = FORMS[form]
    ctx = cs.Context(0)
    try:
        for k, v in (keys if tune is None else tune):
            ctx.set_tuning(k, v)
        kw = {} if nu_range is None else dict(nu_range=nu_range)
        col = _column(ns, nlob, n, np_, ctx, cia, want_tau=False, want_M=want_M, **kw)
        col.run()
        r = dict(form=col.info()["flux_form"], flags=col.work()["dispatch"]["flags"], wts=col.wts.copy(), np=col.np, nnu=col.nnu, cia=cia,
                 nu=col.nu.copy(), Tlev=col.Tlev.copy())
        if want_M is True:
            r["Mup"], r["Mdn"] = np.zeros((col.np, col.nnu), order="F"), np.zeros((col.np, col.nnu), order="F")
            r["Fup"], r["Fdn"] = col.fetch(Mup=r["Mup"], Mdn=r["Mdn"])
        elif want_M == "edges":
            r["Mup"], r["Mdn"] = col.edge_spectra()
            r["Fup"], r["Fdn"] = col.fetch()
        else:
            r["Fup_t"], r["Fdn_t"] = col.tile_fluxes()
            r["Fup"], r["Fdn"] = col.fetch()
    finally:
        ctx.close()
    if tune is None:
        FO._is(r, flux_form, streams=streams, chunk4=chunk4)
    return r


@functools.lru_cache(maxsize=None)                # (36 cases of at most 2 x 9 x 2577 doubles)
def _planes(form, ns, n, np_, nlob, cia):
    """the planes column of a case: the reference of its edges and its tiles test, computed once and left unchanged"""
    r = _one(form, ns, n, np_, nlob, cia, True)
    for k in ("Mup", "Mdn", "Fup", "Fdn"):
        r[k].setflags(write=False)
        assert np.all(np.isfinite(r[k])) and np.all(r[k] > 0.0), k      # (thermal emission and the beam: nothing compared below is a zero)
    return r


def _tile_check(Ft, M, w, F, what):
    """tile sums [np, ntile] against fsum(w_j M[i, j]) over each tile; fsum over a level's tiles against its band flux"""
    npl, nnu = M.shape
    ranges = clearsky_jl_amd.tile_ranges(nnu)
    assert Ft.shape == (npl, len(ranges))
    prod = w[None, :] * M                        # (one rounding per product, as on the device; every term >= 0)
    worst = 0.0
    for i in range(npl):
        for t, (j0, j1) in enumerate(ranges):
            ref = math.fsum(prod[i, j0:j1])
            bound = 66 * U * math.fsum(np.abs(prod[i, j0:j1]))
            err = abs(Ft[i, t] - ref)
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
            assert err <= bound, (what, i, t, Ft[i, t], ref, err, bound)
        tot = math.fsum(Ft[i, :])
        assert abs(tot - F[i]) <= (len(ranges) + 66) * U * F[i], (what, i, tot, F[i])
    print(f"  {what}: {npl} x {len(ranges)} tiles, worst tile error / bound {worst:.3e}")


@pytest.mark.parametrize("form,ns,n,np_,nlob,cia", _cases())
def test_edges_equal_the_planes_rows(form, ns, n, np_, nlob, cia):
    """1. edge_spectra() = rows 0 and np-1 of the planes, Fup and Fdn those of the planes column: to the bit"""
    A = _planes(form, ns, n, np_, nlob, cia)
    E = _one(form, ns, n, np_, nlob, cia, "edges")
    assert (E["form"], E["flags"]) == (A["form"], A["flags"])
    for k in ("Mup", "Mdn"):
        assert E[k].shape == (2, n)
        assert np.array_equal(E[k][0], A[k][0]), (k, "TOA")
        assert np.array_equal(E[k][1], A[k][np_ - 1]), (k, "level np-1")
    assert np.array_equal(E["Fup"], A["Fup"]) and np.array_equal(E["Fdn"], A["Fdn"])


@pytest.mark.parametrize("form,ns,n,np_,nlob,cia", _cases())
def test_tiles_equal_the_planes_sums(form, ns, n, np_, nlob, cia):
    """2. tile_fluxes()[i, t] = fsum(w_j M[i, j]) over the tile within 66 x 2^-53 x sum |w_j M_j|; the band fluxes to the bit; the tiles of
    a level add up to its band flux within (ntile + 66) x 2^-53 x F"""
    A = _planes(form, ns, n, np_, nlob, cia)
    T = _one(form, ns, n, np_, nlob, cia, "tiles")
    assert (T["form"], T["flags"]) == (A["form"], A["flags"])
    assert np.array_equal(T["Fup"], A["Fup"]) and np.array_equal(T["Fdn"], A["Fdn"])
    _tile_check(T["Fup_t"], A["Mup"], A["wts"], A["Fup"], "Fup_t")
    _tile_check(T["Fdn_t"], A["Mdn"], A["wts"], A["Fdn"], "Fdn_t")


@pytest.mark.parametrize("a", [33, 1])
def test_shard_tiles_and_edges_are_the_whole_grid_s(a):
    """3. nu_range = (64 a, 64 b + 17) with b = 40 on the 2577-point grid: the shard starts at a tile boundary inside the grid and ends on
    the grid's ragged tile, its weights are the global trapezoid weights, so its tiles are the whole column's tiles a .. b and its edge
    spectra the whole column's on those points.  Default keys: the form follows the grid size (both are asserted to be the scan form
    here; a = 1 is a shard of 40 tiles, a = 33 one of 8).  The per-point fluxes of two grids agree as two forms do -- the line sums are
    laid out by grid -- so the edge spectra are held to test_gpu_merge._close's 1e-12 of the largest flux + conftest's
    source_rounding_bound, and a tile to the summation bound of test 2 plus that per-point allowance times the tile's weights"""
    n, b, ns, np_, nlob = FO.N_SHORT, 40, 4, 9, 3
    assert n == 64 * b + 17 and 0 < a < b
    rng = (64 * a, 64 * b + 17)
    whole_t = _one("scan5", ns, n, np_, nlob, False, "tiles")
    whole_e = _one("scan5", ns, n, np_, nlob, False, "edges")
    whole_p = _planes("scan5", ns, n, np_, nlob, False)
    shard_t = _one("scan5", ns, n, np_, nlob, False, "tiles", nu_range=rng)
    shard_e = _one("scan5", ns, n, np_, nlob, False, "edges", nu_range=rng)
    assert shard_t["nnu"] == rng[1] - rng[0] and np.array_equal(shard_t["wts"], whole_t["wts"][rng[0]:rng[1]])
    # the optical depths behind source_rounding_bound: a tau column of the whole grid
    cs = clearsky_jl_amd
    ctx = cs.Context(0)
    try:
        col = FO._column(ns, nlob, n, np_, ctx, want_tau=True, want_M=False)
        col.run()
        tau = np.zeros((col.nl, col.nnu), order="F")
        col.fetch(tau=tau)
    finally:
        ctx.close()
    sm = float(np.max(whole_p["Mup"]))
    per_point = 1e-12 * sm + source_rounding_bound(cs, whole_p["nu"], whole_p["Tlev"], tau)
    for k in ("Mup", "Mdn"):
        d = float(np.max(np.abs(shard_e[k] - whole_e[k][:, rng[0]:rng[1]])))
        print(f"  a = {a}: edge spectra {k}: max difference {d:.3e}, allowed {per_point:.3e}")
        assert d < per_point, k
    w = shard_t["wts"]
    for k in ("Fup_t", "Fdn_t"):
        S, Wt = shard_t[k], whole_t[k][:, a:b + 1]
        assert S.shape == Wt.shape == (np_, b + 1 - a)
        worst = 0.0
        for t, (j0, j1) in enumerate(cs.tile_ranges(rng[1] - rng[0])):
            bound = 66 * U * np.abs(Wt[:, t]) + per_point * math.fsum(w[j0:j1])
            err = np.abs(S[:, t] - Wt[:, t])
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (k, t, err, bound)
        print(f"  a = {a}: {k}: worst tile difference / bound {worst:.3e}")


def _raw_column(cs, ctx, ns=4, nlob=2, n=FO.N_SHORT, np_=9):
    """the inputs of a column as the C ABI takes them (Column(_setup=False) evaluates the closures)"""
    return FO._column(ns, nlob, n, np_, ctx, _setup=False)


def _raw_setup(cs, ctx, col, want_M, wts=False):
    """cs_column_setup through ctypes with the given want_M; wts=False: NULL, the trapezoid weights of the column's own grid"""
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int)) if len(a) else None
    rc = cs.lib().cs_column_setup(
        ctx.handle, col.nnu, cs.dptr(col.nu), cs.dptr(col.wts) if wts else None, col.np, cs.dptr(col.P), col.g, col.core.nlobatto,
        cs.dptr(np.asfortranarray(col.Tn).ravel(order="F").copy()), cs.dptr(np.asfortranarray(col.mun).ravel(order="F").copy()),
        cs.dptr(col.Tlev), len(col.gases), ip(col.slots), ip(col.shapes), cs.dptr(col.cuts), cs.dptr(col.conc.ravel(order="F").copy()),
        col.sigma_gray, None, cs.dptr(col.S_toa), cs.dptr(col.albedo), col.theta_s, col.core.nstream, 0, int(want_M))
    ctx._resident = None
    cs.check(rc)


def _raw_fetch(cs, ctx, col, Mup, Mdn):
    Fup, Fdn = np.zeros(col.np), np.zeros(col.np)
    rc = cs.lib().cs_column_fetch(ctx.handle, col.nnu, col.np, None, None if Mup is None else Mup.ctypes.data_as(_dp),
                                  None if Mdn is None else Mdn.ctypes.data_as(_dp), cs.dptr(Fup), cs.dptr(Fdn))
    return rc, Fup, Fdn


def test_update_gives_a_fresh_column_s_edges():
    """4a. an edges column, update() to another temperature profile, run again: what a fresh context returns for that profile"""
    cs = clearsky_jl_amd
    ns, nlob, n, np_ = 4, 3, FO.N_SHORT, 9
    out = []
    for fresh in (False, True):
        ctx = cs.Context(0)
        try:
            col = FO._column(ns, nlob, n, np_, ctx, want_tau=False, want_M="edges")
            T2 = W.earth_temperature(col.P) + np.linspace(-6.0, 9.0, np_)
            if fresh:
                col = cs.Column(col.P, 9.8, T2, 0.029, FO.FS, FO.FA, *FO._members(FO._nu(n)), core=cs.Discretized(ns, nlob), theta_s=FO.THETA_S,
                                ctx=ctx, _warn=False, want_tau=False, want_M="edges")
            else:
                col.run()
                first = col.edge_spectra()
                col.update(T2)
            col.run()
            Mu, Md = col.edge_spectra()
            Fu, Fd = col.fetch()
            assert col.info()["flux_form"] == 3
            out.append((Mu, Md, Fu, Fd))
            if not fresh:
                assert not np.array_equal(first[0], Mu)      # (the profile did change the spectra)
        finally:
            ctx.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_host_pointer_call_never_takes_an_edges_column_for_planes():
    """4b. a resident edges (and then a tiles) column set up exactly as cs_fluxes_discretized sets its own up -- same grid, levels, gases,
    NULL weights, no tau -- then the raw host-pointer call with non-NULL Mup / Mdn on the same context: it compares modes, sets a planes
    column up, and returns the planes of a fresh context to the bit"""
    cs = clearsky_jl_amd
    sl = FO._lines("CO2")

    def call(ctx, col):
        return _julia_call(cs, ctx, col.nu, col.P, col.g, col.core.nlobatto, col.Tn, col.mun, col.Tlev, [sl], ["voigt"], [25.0], col.conc,
                           col.sigma_gray, None, col.S_toa, col.albedo, FO.THETA_S, col.core.nstream, want_tau=False)

    ctx = cs.Context(0)
    try:
        col = _raw_column(cs, ctx)
        ref = call(ctx, col)
    finally:
        ctx.close()
    for mode in (2, 3):
        ctx = cs.Context(0)
        try:
            col = _raw_column(cs, ctx)
            _raw_setup(cs, ctx, col, mode)
            cs.check(cs.lib().cs_column_run(ctx.handle, None))
            shape = (2, col.nnu) if mode == 2 else (col.np, -(-col.nnu // 64))
            bu, bd = np.zeros(col.np * col.nnu), np.zeros(col.np * col.nnu)      # (full-size: a library without the modes overruns nothing)
            rc, Fu, Fd = _raw_fetch(cs, ctx, col, bu, bd)
            cs.check(rc)
            Mu, Md = (b[:shape[0] * shape[1]].reshape(shape, order="F") for b in (bu, bd))
            got = call(ctx, col)
        finally:
            ctx.close()
        for k in ("Mup", "Mdn", "Fup", "Fdn"):
            assert np.array_equal(got[k], ref[k]), (mode, k)
        assert np.array_equal(Fu, ref["Fup"]) and np.array_equal(Fd, ref["Fdn"])
        if mode == 2:
            assert np.array_equal(Mu[0], ref["Mup"][0]) and np.array_equal(Md[1], ref["Mdn"][-1])


def test_edges_under_the_captured_step():
    """4c. key 4: the step is captured on the second run and replayed from the third; three runs of an edges column return the same"""
    cs = clearsky_jl_amd
    ctx = cs.Context(0)
    try:
        ctx.set_tuning(4, 1)
        col = FO._column(4, 2, FO.N_SHORT, 9, ctx, want_tau=False, want_M="edges")
        runs = []
        for _ in range(3):
            col.run()
            runs.append(col.edge_spectra() + col.fetch())
        assert col.info()["flux_form"] == 3
    finally:
        ctx.close()
    ref = _one("scan5", 4, FO.N_SHORT, 9, 2, False, "edges")
    for r in runs:
        for x, y in zip(r, (ref["Mup"], ref["Mdn"], ref["Fup"], ref["Fdn"])):
            assert np.array_equal(x, y)


def test_radiate_with_the_edges_fluxpack():
    """Discretized(fluxpack="edges"): radiate_ fills the boundary rows of F.Mup, F.Mdn (those of a full radiate, to the bit: the same
    kernel) and the band fluxes (1e-14: the full call forms its trapezoid weights on the device), and leaves tau and the inner rows alone"""
    cs = clearsky_jl_amd
    n, np_ = FO.N_SHORT, 9
    nu = FO._nu(n)
    P = cs.pressuregrid(5.0, 1e5, np_)
    ctx = cs.Context(0)
    try:
        args = (P, 9.8, W.earth_temperature(P), 0.029, FO.FS, FO.FA, *FO._members(nu))
        full = cs.radiate(*args, core=cs.Discretized(4, 2), theta_s=FO.THETA_S, ctx=ctx)
        F = cs.FluxPack(np_, n)
        F.tau[:], F.Mup[:], F.Mdn[:] = 7.0, -1.0, -2.0
        cs.radiate_(F, cs.Discretized(4, 2, fluxpack="edges"), *args, theta_s=FO.THETA_S, ctx=ctx)
    finally:
        ctx.close()
    for k in ("Mup", "Mdn"):
        got, ref = getattr(F, k), getattr(full, k)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[-1], ref[-1]), k
    assert np.all(F.tau == 7.0) and np.all(F.Mup[1:-1] == -1.0) and np.all(F.Mdn[1:-1] == -2.0)
    fm = np.max(full.Fup)
    assert np.max(np.abs(F.Fup - full.Fup)) <= 1e-14 * fm and np.max(np.abs(F.Fdn - full.Fdn)) <= 1e-14 * fm
    assert np.array_equal(F.Fnet, F.Fup - F.Fdn)


@pytest.mark.parametrize("n", [FO.N_SHORT, 65])
def test_raw_abi_writes_what_the_mode_says(n):
    """5. cs_column_setup with want_M = 2, 3, 7, 0 through ctypes, then cs_column_fetch into FULL-SIZE [np, nnu] buffers of a sentinel:
    exactly the first 2 nnu (edges) or np ntile (tiles) doubles are written, column-major with the level fastest; 7 still means planes;
    Mup of a want_M = 0 column is CS_ESTATE"""
    cs = clearsky_jl_amd
    np_ = 9
    ntile = -(-n // 64)
    res = {}
    for mode in (1, 2, 3, 7, 0):
        ctx = cs.Context(0)
        try:
            col = _raw_column(cs, ctx, n=n, np_=np_)
            _raw_setup(cs, ctx, col, mode, wts=True)
            cs.check(cs.lib().cs_column_run(ctx.handle, None))
            Mu, Md = np.full(np_ * n, SENTINEL), np.full(np_ * n, SENTINEL)
            rc, Fu, Fd = _raw_fetch(cs, ctx, col, Mu, Md)
            if mode == 0:
                assert rc == CS_ESTATE
                assert np.all(Mu == SENTINEL) and np.all(Md == SENTINEL)
                rc, Fu, Fd = _raw_fetch(cs, ctx, col, None, None)
            cs.check(rc)
            res[mode] = (Mu, Md, Fu, Fd)
        finally:
            ctx.close()
    P1 = [a.reshape((np_, n), order="F") for a in res[1][:2]]
    for a in P1:
        assert not np.any(a == SENTINEL)
    for mode, used in ((2, 2 * n), (3, np_ * ntile)):
        for a, plane in zip(res[mode][:2], P1):
            assert not np.any(a[:used] == SENTINEL), mode
            assert np.all(a[used:] == SENTINEL), (mode, int(np.sum(a[used:] != SENTINEL)))
            if mode == 2:
                e = a[:used].reshape((2, n), order="F")
                assert np.array_equal(e[0], plane[0]) and np.array_equal(e[1], plane[np_ - 1])
            else:
                t = a[:used].reshape((np_, ntile), order="F")
                prod = col.wts[None, :] * plane
                for q, (j0, j1) in enumerate(cs.tile_ranges(n)):
                    s = np.array([math.fsum(prod[i, j0:j1]) for i in range(np_)])
                    assert np.all(np.abs(t[:, q] - s) <= 66 * U * s), (q, t[:, q], s)
    for k in range(4):
        assert np.array_equal(res[7][k], res[1][k]), k            # any other non-zero value: planes
    for mode in (2, 3, 0):
        assert np.array_equal(res[mode][2], res[1][2]) and np.array_equal(res[mode][3], res[1][3]), mode
