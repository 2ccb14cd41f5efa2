"""The two reduced forms of the optical depths of a resident column -- want_tau="total" (the slant optical depth of the whole column,
[nnu], no floor) and want_tau="tiles" (sum of w_j exp(-D_i(nu_j)) over every 64-point tile, [np, ntile]) -- that k_depth
(cs_kernels.h) forms from the finished cross-section plane, after cs_column_run and after cs_column_sigma_run.

Reference and bound: tests/depth_ref.py -- 40-digit values on the doubles the device was given (the plane Column.sigma_nodes() returns
after the same call, the column's muk, P, weights and Lobatto weights), a counted first-order bound per element.  k_depth calls the
library's exponential: E = flux_ref.E_EXP["libm"].  Every element of every case must lie inside the bound.

  1. kernel alone: gas-free columns whose plane is flux_ref.sigma_plane (S_FULL: column depths 7e-8 .. 9e3) as sigma_extra
  2. real members: tests/test_gpu_flux_orders.py's column -- the near-line plane kept apart (key 7 = 2) and folded (key 7 = 0), a baked
     table, an accelerated absorber, a code-6 gas after sigma_run (the clamped plane)
  3. the form rule: a total column runs form 0 under every set of keys, its fluxes are bitwise a form-0 column's; other columns keep
     their form and launch count
  4. the raw ABI: what cs_column_fetch writes per mode; the host-pointer entry point after a resident total column
  5. nu-shards cut at a multiple of 64 points  6. update()  7. opticaldepth / transmittance / band_transmittance end to end
"""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest

import clearsky_jl_amd
import depth_ref as DR
import flux_ref as F
import workloads as W
import test_gpu_flux_orders as FO
import test_gpu_reduced_spectra as RS
from test_gpu_boundary import _julia_call
from test_gpu_flux_ref import _absorber

pytestmark = pytest.mark.gpu

U = F.U
CS_ESTATE = -6
SENTINEL = -7.25e300                             # (no depth and no transmittance is negative)
_dp = C.POINTER(C.c_double)
_REF = {}


def _reference(col, sig, theta):
    """depth_ref.mp_depth + bounds on the plane a column returned, kept by the plane's content (the total and the tiles column of a
    case return the same plane)"""
    h = hashlib.sha1()
    for a in (sig, col.muk, col.P, col.wts):
        h.update(np.ascontiguousarray(a).tobytes())
    key = (h.hexdigest(), float(theta), col.core.nlobatto, col.g)
    if key not in _REF:
        if len(_REF) >= 8:
            _REF.clear()
        ws = clearsky_jl_amd.lobattonodes(col.core.nlobatto)[1]
        ref = DR.mp_depth(col.P, col.g, col.muk, sig, theta, ws, wts=col.wts)
        _REF[key] = (ref, DR.bounds(ref))
    return _REF[key]


def _get(col, mode):
    return col.column_depth() if mode == "total" else col.tile_transmittance()


def _held(col, mode, theta, what):
    """fetch the column's product, then the plane it was formed from; every element inside the bound.  Returns (got, reference as doubles)"""
    got = _get(col, mode)
    sig = col.sigma_nodes()
    ref, bnd = _reference(col, sig, theta)
    if mode == "total":
        r = F.ratio(got, ref["D"][-1], bnd["D"][-1])
        exact = F.to_float(ref["D"][-1])
    else:
        assert got.shape == (col.np, col.ntile)
        r = F.ratio(got, ref["T"], bnd["T"])
        exact = F.to_float(ref["T"])
    print(f"  {what} {mode}: worst error / bound {r:.3f}")
    assert r <= 1.0, (what, mode, r)
    return got, exact


def _run(col, after):
    col.run() if after == "run" else col.sigma_run()


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("np_,nlob", [(2, 2), (9, 3), (9, 2), (2, 4)])
@pytest.mark.parametrize("n", [17, 64, 65, 145])
def test_kernel_alone(n, np_, nlob):
    cs = clearsky_jl_amd
    ctx = cs.Context(0)
    try:
        for theta in (0.0, 0.6):
            c = DR.case(cs, nlob, np_, nnu=n, theta=theta)
            for mode in ("total", "tiles"):
                for after in ("run", "sigma_run"):
                    col = cs.Column(c["P"], c["g"], c["T"], F.fmu, None, None, cs.GrayGas(0.0, c["nu"]), _absorber(c),
                                    core=cs.Discretized(4, nlob), theta_s=theta, want_tau=mode, want_M=False, ctx=ctx, _warn=False)
                    assert np.array_equal(col.muk, c["muk"]) and col.sigma_gray == 0.0
                    _run(col, after)
                    got, exact = _held(col, mode, theta, f"n={n} np={np_} nlob={nlob} theta={theta} after {after}")
                    assert np.array_equal(col.sigma_nodes(), c["sigma"])             # the reference's input is the case's plane, exactly
                    if mode == "total":
                        assert got.shape == (n,) and got.min() < 0.2 * (np_ - 1) * 1e-6    # no floor: nl layers on it would give nl x 1e-6
                    else:
                        assert np.all(got[0] == pytest.approx([math.fsum(col.wts[a:b]) for a, b in cs.tile_ranges(n)], rel=66 * U))
                    if after == "run":
                        assert col.info()["flux_form"] == 0
    finally:
        ctx.close()


# ---- 2. real members -------------------------------------------------------------------------------------------------------------

def _real(kind, ctx, n, mode):
    """a column of tests/test_gpu_flux_orders.py's kind (CO2 line by line, gray term, CIA pair, beam, albedo; np = 9), or one of its
    variants: the same members behind a baked table / an accelerated absorber / under shape code 6"""
    cs = clearsky_jl_amd
    nu = FO._nu(n)
    P = cs.pressuregrid(5.0, 1e5, 9)
    T = W.earth_temperature(P)
    kw = dict(core=cs.Discretized(4, 3), theta_s=FO.THETA_S, want_tau=mode, want_M=False, ctx=ctx, _warn=False)
    if kind in ("apart", "folded"):
        ctx.set_tuning(7, 2 if kind == "apart" else 0)
        return FO._column(4, 3, n, 9, ctx, cia=True, want_tau=mode, want_M=False)
    if kind == "baked":
        Om = cs.AtmosphericDomain((180.0, 320.0), 5, (1.0, 1.2e5), 6)
        g = cs.Gas(FO._lines("CO2"), 400e-6, nu, Om, ctx=ctx)
        return cs.Column(P, 9.8, T, 0.029, FO.FS, FO.FA, g, cs.GrayGas(FO.GRAY, nu), **kw)
    if kind == "accel":
        Pk = cs.pressuregrid(4.0, 1.1e5, 7)
        A = cs.AcceleratedAbsorber(W.earth_temperature(Pk), Pk, *FO._members(nu), ctx=ctx)
        return cs.Column(P, 9.8, T, 0.029, FO.FS, FO.FA, A, **kw)
    assert kind == "code6"
    return cs.Column(P, 9.8, T, 0.029, FO.FS, FO.FA, cs.DirectGas(FO._lines("CO2"), 400e-6, nu, shape="voigtCKDVVH"),
                     cs.GrayGas(FO.GRAY, nu), **kw)


@pytest.mark.parametrize("kind,n,after", [("apart", FO.N_SHORT, "run"), ("folded", FO.N_SHORT, "run"), ("folded", 65, "sigma_run"),
                                          ("apart", 65, "run"), ("baked", 65, "run"), ("accel", FO.N_SHORT, "run"), ("accel", 65, "sigma_run"),
                                          ("code6", FO.N_SHORT, "sigma_run"), ("code6", 65, "run")])
def test_real_members(kind, n, after):
    cs = clearsky_jl_amd
    for mode in ("total", "tiles"):
        ctx = cs.Context(0)
        try:
            col = _real(kind, ctx, n, mode)
            _run(col, after)
            if after == "run":
                assert col.info()["flux_form"] == 0
                streams = col.work()["dispatch"]["streams"]
                if kind == "apart" and n == FO.N_SHORT:
                    assert streams & 2, streams                     # the near-line pairs in a plane of their own: k_depth read both
                if kind == "folded":
                    assert not streams & 2, streams
            got, exact = _held(col, mode, FO.THETA_S, f"{kind} n={n} after {after}")
            if mode == "total":
                assert got.shape == (n,) and np.all(got > 0.0)
            if kind == "code6" and after == "sigma_run":
                assert np.all(col.sigma_nodes() >= 0.0)             # the clamped plane
        finally:
            ctx.close()


# ---- 3. the form rule ------------------------------------------------------------------------------------------------------------

def _form_column(keys, want_tau, ns=4, nlob=2, n=FO.N_SHORT, np_=9):
    cs = clearsky_jl_amd
    ctx = cs.Context(0)
    try:
        for k, v in keys:
            ctx.set_tuning(k, v)
        col = FO._column(ns, nlob, n, np_, ctx, want_tau=want_tau, want_M="edges")
        col.run()
        Mu, Md = col.edge_spectra()
        Fu, Fd = col.fetch()
        return dict(form=col.info()["flux_form"], launches=col.info()["launches"], flags=col.work()["dispatch"]["flags"], Mup=Mu, Mdn=Md,
                    Fup=Fu, Fdn=Fd)
    finally:
        ctx.close()


@pytest.mark.parametrize("form", list(RS.FORMS))
def test_form_rule(form):
    keys, flux_form, streams, chunk4, _ = RS.FORMS[form]
    zero = tuple(kv for kv in keys if kv[0] != 15) + ((15, 1),)      # the same keys with the flux stage forced to the separate kernels
    Tt = _form_column(keys, "total")
    Z = _form_column(zero, False)
    assert Tt["form"] == 0 and Z["form"] == 0
    assert Tt["flags"] == Z["flags"]
    for k in ("Fup", "Fdn", "Mup", "Mdn"):
        assert np.array_equal(Tt[k], Z[k]), k
    assert Tt["launches"] == Z["launches"] + 1                      # k_depth
    # every other column: the form these keys have always given, want_tau or not, and one launch count
    A, B = _form_column(keys, False), _form_column(keys, True)
    for r in (A, B):
        FO._is(r, flux_form, streams=streams, chunk4=chunk4)
    assert A["launches"] == B["launches"]
    if flux_form == 0:
        assert A["launches"] == Z["launches"]


# ---- 4. plumbing through ctypes --------------------------------------------------------------------------------------------------

def _raw_setup(cs, ctx, col, want_tau):
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int)) if len(a) else None
    rc = cs.lib().cs_column_setup(
        ctx.handle, col.nnu, cs.dptr(col.nu), None, col.np, cs.dptr(col.P), col.g, col.core.nlobatto,
        cs.dptr(np.asfortranarray(col.Tn).ravel(order="F").copy()), cs.dptr(np.asfortranarray(col.mun).ravel(order="F").copy()),
        cs.dptr(col.Tlev), len(col.gases), ip(col.slots), ip(col.shapes), cs.dptr(col.cuts), cs.dptr(col.conc.ravel(order="F").copy()),
        col.sigma_gray, None, cs.dptr(col.S_toa), cs.dptr(col.albedo), col.theta_s, col.core.nstream, int(want_tau), 0)
    ctx._resident = None
    cs.check(rc)


@pytest.mark.parametrize("n", [FO.N_SHORT, 65])
def test_raw_abi_writes_what_the_mode_says(n):
    cs = clearsky_jl_amd
    np_ = 9
    ntile = -(-n // 64)
    res = {}
    for mode in (2, 3, 1, 7, 0):
        ctx = cs.Context(0)
        try:
            col = RS._raw_column(cs, ctx, n=n, np_=np_)
            _raw_setup(cs, ctx, col, mode)
            cs.check(cs.lib().cs_column_run(ctx.handle, None))
            buf = np.full(np_ * n, SENTINEL)
            Fu, Fd = np.zeros(np_), np.zeros(np_)
            rc = cs.lib().cs_column_fetch(ctx.handle, n, np_, buf.ctypes.data_as(_dp), None, None, cs.dptr(Fu), cs.dptr(Fd))
            if mode == 0:
                assert rc == CS_ESTATE and np.all(buf == SENTINEL)
            else:
                cs.check(rc)
            res[mode] = buf
        finally:
            ctx.close()
    for mode, used in ((2, n), (3, np_ * ntile), (1, (np_ - 1) * n), (7, (np_ - 1) * n)):
        a = res[mode]
        assert not np.any(a[:used] == SENTINEL), mode
        assert np.all(a[used:] == SENTINEL), (mode, int(np.sum(a[used:] != SENTINEL)))
    assert np.array_equal(res[7], res[1])                            # any other non-zero value: layers
    t = res[3][:np_ * ntile].reshape((np_, ntile), order="F")        # level fastest
    assert np.all(np.diff(t, axis=0) < 0.0) and np.all(t[0] == pytest.approx([math.fsum(col.wts[a:b]) for a, b in cs.tile_ranges(n)], rel=66 * U))
    assert np.all(res[2][:n] > 0.0) and np.all(res[1][:(np_ - 1) * n] >= 1e-6)


def test_host_pointer_call_never_takes_a_total_column_for_layers():
    cs = clearsky_jl_amd
    sl = FO._lines("CO2")

    def call(ctx, col):
        return _julia_call(cs, ctx, col.nu, col.P, col.g, col.core.nlobatto, col.Tn, col.mun, col.Tlev, [sl], ["voigt"], [25.0], col.conc,
                           col.sigma_gray, None, col.S_toa, col.albedo, FO.THETA_S, col.core.nstream, want_tau=True, want_M=False)

    ctx = cs.Context(0)
    try:
        col = RS._raw_column(cs, ctx)
        ref = call(ctx, col)
    finally:
        ctx.close()
    for mode in (2, 3):
        ctx = cs.Context(0)
        try:
            col = RS._raw_column(cs, ctx)
            _raw_setup(cs, ctx, col, mode)
            cs.check(cs.lib().cs_column_run(ctx.handle, None))
            got = call(ctx, col)
        finally:
            ctx.close()
        for k in ("tau", "Fup", "Fdn"):
            assert np.array_equal(got[k], ref[k]), (mode, k)


# ---- 5. shards -------------------------------------------------------------------------------------------------------------------

def test_shards_cut_at_a_tile_boundary():
    """two nu_range shards cut at point 128 of a 209-point grid (three whole tiles and a ragged one), with slices of the global weights,
    on flux_ref's S_FULL plane handed in as a function absorber (a plane that does not depend on how a grid lays out its line sums): the
    points and the tiles of the whole column, bitwise -- a shard's tile holds the same points in the same lanes"""
    cs = clearsky_jl_amd
    n, cut, np_, nlob, theta = 64 * 3 + 17, 128, 9, 3, 0.6
    c = DR.case(cs, nlob, np_, nnu=n, theta=theta)
    row = {float(p): k for k, p in enumerate(c["Pk"])}
    plane = lambda v, T, P: c["sigma"][row[float(P)]][np.searchsorted(c["nu"], v)]
    out = {}
    for mode in ("total", "tiles"):
        for name, rng in (("whole", None), ("lo", (0, cut)), ("hi", (cut, n))):
            ctx = cs.Context(0)
            try:
                kw = {} if rng is None else dict(nu_range=rng)
                col = cs.Column(c["P"], c["g"], c["T"], F.fmu, None, None, cs.GrayGas(0.0, c["nu"]), plane, core=cs.Discretized(4, nlob),
                                theta_s=theta, want_tau=mode, want_M=False, ctx=ctx, _warn=False, **kw)
                col.sigma_run()
                out[mode, name] = _get(col, mode)
                out["wts", name] = col.wts.copy()
                if rng is None:
                    assert np.array_equal(col.sigma_nodes(), c["sigma"])
                    _held(col, mode, theta, "whole grid of the shard test")
            finally:
                ctx.close()
    assert np.array_equal(np.concatenate([out["wts", "lo"], out["wts", "hi"]]), out["wts", "whole"])
    assert out["total", "lo"].shape == (cut,) and out["total", "hi"].shape == (n - cut,)
    assert np.array_equal(np.concatenate([out["total", "lo"], out["total", "hi"]]), out["total", "whole"])
    assert out["tiles", "lo"].shape == (np_, 2) and out["tiles", "hi"].shape == (np_, 2) and out["tiles", "whole"].shape == (np_, 4)
    assert np.array_equal(np.concatenate([out["tiles", "lo"], out["tiles", "hi"]], axis=1), out["tiles", "whole"])


# ---- 6. update -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["total", "tiles"])
def test_update_gives_a_fresh_column_s_depths(mode):
    cs = clearsky_jl_amd
    ns, nlob, n, np_ = 4, 3, FO.N_SHORT, 9
    out = []
    for fresh in (False, True):
        ctx = cs.Context(0)
        try:
            col = FO._column(ns, nlob, n, np_, ctx, want_tau=mode, want_M=False)
            T2 = W.earth_temperature(col.P) + np.linspace(-6.0, 9.0, np_)
            if fresh:
                col = cs.Column(col.P, 9.8, T2, 0.029, FO.FS, FO.FA, *FO._members(FO._nu(n)), core=cs.Discretized(ns, nlob), theta_s=FO.THETA_S,
                                ctx=ctx, _warn=False, want_tau=mode, want_M=False)
            else:
                col.run()
                first = _get(col, mode)
                col.update(T2)
            col.run()
            out.append((_get(col, mode),) + col.fetch())
            assert col.info()["flux_form"] == 0
            if not fresh:
                assert not np.array_equal(first, out[0][0])          # (the profile did change the depths)
        finally:
            ctx.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_total_under_the_captured_step():
    """key 4: the step is captured on the second run and replayed from the third; k_depth is part of it"""
    cs = clearsky_jl_amd
    ctx = cs.Context(0)
    try:
        ctx.set_tuning(4, 1)
        col = FO._column(4, 2, FO.N_SHORT, 9, ctx, want_tau="total", want_M=False)
        runs = []
        for _ in range(3):
            col.run()
            runs.append(col.column_depth())
    finally:
        ctx.close()
    assert np.all(runs[0] > 0.0) and np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------

def test_opticaldepth_end_to_end():
    """opticaldepth / transmittance against the formula the package evaluated on the host before k_depth existed, on the plane the same
    column returns (depth_ref.host_formula), inside the D bound of both; band_transmittance over all tiles of a level"""
    cs = clearsky_jl_amd
    n, theta, nlob = 2577, 0.6, 4
    nu = FO._nu(n)
    P = cs.pressuregrid(5.0, 1e5, 9)
    T = W.earth_temperature(P)
    ctx = cs.Context(0)
    try:
        members = FO._members(nu, cia=True)
        D = cs.opticaldepth(P, 9.8, T, 0.029, theta, *members, nlobatto=nlob, ctx=ctx)
        col = ctx._resident
        assert col.tau_mode == 2 and col.theta_s == theta and col.core.nlobatto == nlob
        sig = col.sigma_nodes()
        ws = cs.lobattonodes(nlob)[1]
        host = DR.host_formula(col.P, col.g, col.muk, sig, theta, ws)
        ref, bnd = _reference(col, sig, theta)
        for what, a in (("device", D), ("host formula", host)):
            r = F.ratio(a, ref["D"][-1], bnd["D"][-1])
            print(f"  opticaldepth, {what}: worst error / bound {r:.3f}")
            assert r <= 1.0, what
        assert np.all(np.abs(D - host) <= 2.0 * bnd["D"][-1])           # (results move by rounding only)
        t = cs.transmittance(P, 9.8, T, 0.029, theta, *members, nlobatto=nlob, ctx=ctx)
        assert np.array_equal(t, np.exp(-D))
        colt = cs.Column(P, 9.8, T, 0.029, None, None, *members, core=cs.Discretized(5, nlob), theta_s=theta, want_tau="tiles", want_M=False,
                         ctx=ctx, _warn=False)
        colt.sigma_run()
        Tt = colt.tile_transmittance()
    finally:
        ctx.close()
    ntile = Tt.shape[1]
    B = cs.band_transmittance(Tt, [0, ntile])
    assert B.shape == (9, 1)
    for i in range(9):
        want = math.fsum(Tt[i]) / math.fsum(Tt[0])
        assert abs(B[i, 0] - want) <= (ntile + 66) * U * want, i
    assert B[0, 0] == 1.0 and np.all(np.diff(B[:, 0]) < 0.0)
