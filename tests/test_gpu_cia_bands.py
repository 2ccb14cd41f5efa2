"""CIA bands on synthetic tables, every flux form: columns whose cross-section is the CIA term alone, so that the optical depth is a sharp
probe of the arithmetic fused into the flux kernels (k_cia_tab + cia_add in k_flux_scan / k_flux_chunk*) as well as of the separate
k_cia.  The line gas the fused forms and the pairing need is the CO2 fixture on a grid above its last line + 25 cm^-1 (no line is
included); the synthetic "CO2-CO2" / "CO2-CH4" bands of tests/tabulated_ref.py sit there.

Every case asserts which form ran (Column.info()["flux_form"]: 3 scan, 2 chunk, 0 separate kernels; Column.work()["dispatch"]["flags"]:
RT_STREAMS = 4 for k_rt_streams under the separate kernels, CHUNK4 = 32 never) and that a good share of the reference's layer optical
depths lies above the 1e-6 floor, where both sides would agree trivially.  It compares each form with the
40-digit reference (tabulated_ref.cia_sigma; optical depths and fluxes through the oracle's depth and sweeps fed those cross-sections)
and the forms with each other.  Tolerances: sigma and tau 4 x tabulated_ref.cia_bound (derived there from max |ln k| of the case);
fluxes 1e-11 of the column maximum + conftest.source_rounding_bound's term per wavenumber (_amp).  Each case prints its largest error / bound ratio (pytest -s).
"""
import ctypes as C

import numpy as np
import pytest

import tabulated_ref as R
from clearsky_jl_amd import DISPATCH_FLAGS

pytestmark = pytest.mark.gpu

SCAN, CHUNK, SEP = (), ((15, 2), (5, 0)), ((15, 1),)
FORMS = (("scan", SCAN, 3), ("chunk", CHUNK, 2), ("separate", SEP, 0))
G = 9.8
RT_STREAMS, CHUNK4 = DISPATCH_FLAGS["RT_STREAMS"], DISPATCH_FLAGS["CHUNK4"]   # Column.work()["dispatch"]["flags"]


def _is(r, form, tune):
    """the form, and the flags that go with it on these short grids (tests/test_gpu_flux_orders.py): k_rt_streams whenever the separate
    kernels run with key 5 left on, the four-wave chunk form never"""
    assert r["form"] == form, (r["form"], form)
    assert bool(r["flags"] & RT_STREAMS) == (form == 0 and (5, 0) not in tune), r["flags"]
    assert not r["flags"] & CHUNK4, r["flags"]


def _above_floor(ref, share=0.1):
    f = float((ref["tau"] > 1e-6).mean())
    print(f"  layer optical depths above the floor: {f:.2f}")
    assert f >= share, f


def _profile(np_, lo=150.0, hi=370.0):
    """level temperatures crossing every synthetic band's range [180, 340] (and the narrower ones), with levels exactly on the first, an
    interior and the last temperature knot"""
    T = np.linspace(lo, hi, np_)
    for knot in (180.0, 260.0, 340.0):
        T[int(np.argmin(np.abs(T - knot)))] = knot
    return T


def _outputs(col):
    tau = np.zeros((col.nl, col.nnu), order="F")
    Mu = np.zeros((col.np, col.nnu), order="F")
    Md = np.zeros((col.np, col.nnu), order="F")
    Fup, Fdn = col.fetch(tau, Mu, Md)
    return dict(tau=tau, Mup=Mu, Mdn=Md, Fup=Fup, Fdn=Fdn, form=col.info()["flux_form"], flags=col.work()["dispatch"]["flags"])


def _column(cs, lines, ctx, nu, pairs, np_, nlob, T=None, extrap=False, singles=False, ns=4):
    """pairs: list of (data, symbol); a CO2 (and, for CO2-CH4, a CH4) line gas with no line within reach of the grid"""
    P = cs.pressuregrid(50.0, 1e5, np_)
    gases = [cs.DirectGas(lines("CO2"), 0.9, nu)]
    assert gases[0].sl.nu.max() + 25.0 < nu[0]
    if any(sym == "CO2-CH4" for _, sym in pairs):
        gases.append(cs.DirectGas(lines("CH4"), lambda T_, P_: 0.05 * (P_ / 1e5) ** 0.2, nu))
    xs = [cs.CIATables(d, extrapolate=extrap, singles=singles) for d, _ in pairs]
    return cs.Column(P, G, _profile(np_) if T is None else T, 0.044, 0.0, 0.0, *gases, *xs, core=cs.Discretized(ns, nlob), ctx=ctx, _warn=False)


def _run(cs, lines, nu, pairs, np_, nlob, tune, **kw):
    ctx = cs.Context(0)
    try:
        for k, v in tune:
            ctx.set_tuning(k, v)
        col = _column(cs, lines, ctx, nu, pairs, np_, nlob, **kw)
        col.run()
        r = _outputs(col)
        r["sigma"] = col.sigma_nodes()
        r["col"] = col
    finally:
        ctx.close()
    return r


def _sigma_ref(col, pairs, extrap, singles, P1=None, P2=None, Tk=None):
    P1 = col.cia_P1 if P1 is None else P1
    P2 = col.cia_P2 if P2 is None else P2
    Tk = col.Tk if Tk is None else Tk
    out = np.zeros((col.K, col.nnu))
    for ci, (d, _) in enumerate(pairs):
        for k in range(col.K):
            out[k] += R.cia_sigma(d, col.nu, Tk[k], col.Pk[k], P1[ci, k], P2[ci, k], extrap, singles)
    return out


def _reference(O, col, sig):
    with np.errstate(invalid="ignore"):
        return O.fluxes_discretized(col.nu, col.P, col.g, col.core.nlobatto, col.Tn, col.mun, col.Tlev, [g.sl for g in col.gases],
                                    ["voigt"] * len(col.gases), list(col.cuts), col.conc, sigma_extra=sig, nstream=col.core.nstream,
                                    theta_s=col.theta_s)


def _ratio(a, b, bound):
    """largest |a - b| / (|b| bound) over b != 0; a must be exactly 0 where b is"""
    z = b == 0.0
    assert np.array_equal(a[z], b[z]), "a term where the reference has none"
    return float(np.max(np.abs(a[~z] - b[~z]) / np.abs(b[~z]))) / bound if (~z).any() else 0.0


def _amp(cs, nu, Tlev, tau):
    """the term of conftest.source_rounding_bound -- pi |dB| 2^-53 / tau summed over the layers -- kept per wavenumber instead of its
    maximum over the grid: the floored layers of the points no band reaches would otherwise set the tolerance of every point"""
    B = cs.planck(np.asarray(nu)[None, :], np.asarray(Tlev)[:, None])
    return np.sum(np.pi * np.abs(np.diff(B, axis=0)) * 2.0 ** -53 / np.asarray(tau), axis=0)


def _layer_nan(sig, nlob):
    """a layer's optical depth is NaN where any of its nodes' cross-sections is"""
    n = np.isnan(sig)
    return np.array([np.any(n[i * (nlob - 1): (i + 1) * (nlob - 1) + 1], axis=0) for i in range((sig.shape[0] - 1) // (nlob - 1))])


def _check(cs, r, sig, ref, bands, nlob, label, fluxes=True):
    bs, bt = R.cia_bound(bands), R.cia_bound(bands, nlob)
    assert bt < 1e-12
    nan_s, nan_t = np.isnan(sig), _layer_nan(sig, nlob)
    assert np.array_equal(np.isnan(r["sigma"]), nan_s), label
    assert np.array_equal(np.isnan(r["tau"]), nan_t), label
    rs = _ratio(r["sigma"][~nan_s], sig[~nan_s], bs)
    rt = _ratio(r["tau"][~nan_t], ref["tau"][~nan_t], bt)
    print(f"  {label}: form {r['form']}  sigma err/bound {rs:.3f}  tau err/bound {rt:.3f}")
    assert rs <= 4.0 and rt <= 4.0, (label, rs, rt)
    if fluxes and not nan_s.any():
        sm = max(ref["Mup"].max(), ref["Mdn"].max())
        amp = _amp(cs, r["col"].nu, r["col"].Tlev, ref["tau"])
        for k in ("Mup", "Mdn"):
            assert np.all(np.abs(r[k] - ref[k]) < 1e-11 * sm + amp[None, :]), (label, k)
        for k in ("Fup", "Fdn"):
            assert np.max(np.abs(r[k] - ref[k])) < 1e-11 * ref["Fup"].max(), (label, k)
    return nan_t


def _case(cs, O, lines, nu, pairs, np_, nlob, fused=True, extrap=False, singles=False, forms=FORMS, T=None):
    """one band set through the forms its grid can take; each against the reference, then against the first one"""
    bands = sum((d for d, _ in pairs), [])
    res, sig, ref = [], None, None
    for name, tune, form in forms:
        r = _run(cs, lines, nu, pairs, np_, nlob, tune, extrap=extrap, singles=singles, T=T)
        _is(r, form if fused else 0, tune)
        if sig is None:
            sig = _sigma_ref(r["col"], pairs, extrap, singles)
            ref = _reference(O, r["col"], sig)
            _above_floor(ref)
        nan_t = _check(cs, r, sig, ref, bands, nlob, name)
        res.append(r)
    bt = R.cia_bound(bands, nlob)
    for r in res[1:]:
        assert _ratio(r["tau"][~nan_t], res[0]["tau"][~nan_t], bt) <= 4.0
        if not np.isnan(sig).any():
            amp = _amp(cs, nu, r["col"].Tlev, ref["tau"])
            sm = max(ref["Mup"].max(), ref["Mdn"].max())
            assert np.all(np.abs(r["Mup"] - res[0]["Mup"]) < 1e-11 * sm + amp[None, :])
    return res, sig, ref


# ---- 1, 2: bands per tile --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,np_,nlob", [(1, 6, 2), (2, 9, 3), (3, 10, 3), (4, 12, 3)])
def test_overlap_fused(cs, O, lines, n, np_, nlob):
    """1..4 bands of one object on a tile (slots q = 0..3 of cia_add), bands of 2, 7, 40 and 300 samples with their own temperature grids;
    K = 6, 17, 19, 23: past one 16-state load and not a multiple of 8"""
    nu = R.grid(200)
    data = R.overlap_set(n)
    assert max(R.tile_overlaps(data, nu)) == n
    res, sig, _ = _case(cs, O, lines, nu, [(data, "CO2-CO2")], np_, nlob)
    assert res[0]["col"].K == (np_ - 1) * (nlob - 1) + 1 and sig.max() > 0
    if n >= 3:
        assert res[0]["col"].K > 16 and res[0]["col"].K % 8


@pytest.mark.parametrize("which", ["overlap5", "bands24"])
def test_more_bands_than_the_flux_kernel_holds(cs, O, lines, which):
    """five bands on one tile, and an object of CS_MAX_CIA_BAND = 24 bands: the column drops to the separate kernels (form 0) under every
    key, same tolerance"""
    nu = R.grid(200)
    data = R.overlap_set(5) if which == "overlap5" else R.many_bands(24)
    assert max(R.tile_overlaps(data, nu)) > 4
    _case(cs, O, lines, nu, [(data, "CO2-CO2")], 10, 3, fused=False)


def test_25_bands_refused(cs):
    ctx = cs.Context(0)
    try:
        assert cs.lib().cs_cia_begin(ctx.handle, 0, 24) == 0
        assert cs.lib().cs_cia_begin(ctx.handle, 0, 25) == -1
        with pytest.raises(cs.ClearSkyHIPError):
            ctx.cia_slot(cs.CIATables(R.many_bands(25)))
    finally:
        ctx.close()


# ---- 3, 4: band ends and grids ---------------------------------------------------------------------------------------------------------

def test_band_ends(cs, O, lines):
    """ends on grid points, on a tile's first and last point, bands between two points and between two tiles, a band wider than the grid,
    ends one ulp inside grid points"""
    nu = R.grid(193)
    data = R.ends_set(nu)
    res, sig, _ = _case(cs, O, lines, nu, [(data, "CO2-CO2")], 10, 3)
    k = int(np.argmin(np.abs(res[0]["col"].Tk - 260.0)))
    # (the wide band covers everything; the others add on their own points only)
    wide = R.band(nu[0] - 7.0, nu[-1] + 9.0, 33, R.TS, 5)
    alone = R.cia_sigma(wide, nu, res[0]["col"].Tk[k], res[0]["col"].Pk[k], res[0]["col"].cia_P1[0, k], res[0]["col"].cia_P2[0, k])
    more = np.nonzero(sig[k] > alone * (1 + 1e-9))[0]
    assert set(more) == set(range(5, 21)) | set(range(41, 50)) | set(range(64, 128))


@pytest.mark.parametrize("nnu", [63, 64, 65, 129])
def test_ragged_grids(cs, O, lines, nnu):
    nu = R.grid(nnu)
    data = R.band(nu[0] - 0.1, nu[min(nnu - 1, 70)] + 0.01, 9, R.TS, 1) + R.band(nu[nnu // 2], nu[-1], 5, R.TS[1:4], 2) + R.band(nu[-1], nu[-1] + 3.0, 4, R.TS, 3)
    _case(cs, O, lines, nu, [(data, "CO2-CO2")], 9, 3)


def test_jittered_grid(cs, O, lines):
    rng = np.random.default_rng(7)
    nu = R.NU0 + np.cumsum(rng.uniform(0.02, 0.5, 150))
    data = R.band(nu[3], nu[90], 17, R.TS, 1) + R.band(nu[60] + 0.001, nu[149] - 0.001, 30, R.TS[:3], 2) + R.band(nu[64], nu[127], 3, R.TS, 3)
    _case(cs, O, lines, nu, [(data, "CO2-CO2")], 10, 3)


def test_single_point_grid(cs, O, lines):
    """a grid of one point is accepted (its trapezoid weight is zero: the band fluxes are): sigma and tau of every form"""
    nu = R.grid(1)
    data = R.band(nu[0] - 1.0, nu[0] + 1.0, 5, R.TS, 1)
    for name, tune, form in FORMS:
        r = _run(cs, lines, nu, [(data, "CO2-CO2")], 9, 3, tune)
        _is(r, form, tune)
        sig = _sigma_ref(r["col"], [(data, "CO2-CO2")], False, False)
        ref = _reference(O, r["col"], sig)
        _above_floor(ref)
        _check(cs, r, sig, ref, data, 3, "one point, " + name, fluxes=False)
        assert np.all(r["Fup"] == 0.0) and np.all(r["Fdn"] == 0.0)


# ---- 5: temperatures -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extrap", [False, True])
def test_states_on_both_sides_of_the_temperature_range(cs, O, lines, extrap):
    """node temperatures from 150 to 370 K over bands on 180..220, 180..260, 180..340 and a two-temperature band: some states in, some
    out (the per-state `use`), clamped to the ends under `extrapolate`; levels exactly on the knots 180, 260 and 340 K"""
    nu = R.grid(150)
    data = R.overlap_set(3) + R.band(nu[0] + 0.01, nu[40], 6, (200.0, 300.0), 9)
    res, sig, _ = _case(cs, O, lines, nu, [(data, "CO2-CO2")], 10, 3, extrap=extrap)
    Tk = res[0]["col"].Tk
    assert all(t in Tk for t in (180.0, 260.0, 340.0)) and Tk.min() < 180.0 and Tk.max() > 340.0
    out = (Tk < 180.0) | (Tk > 340.0)
    assert np.all((sig[out] > 0).any(axis=1) == extrap) and np.all((sig[~out] > 0).any(axis=1))


# ---- 6: single-temperature ranges -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("singles", [False, True])
def test_single_ranges_with_zero_samples(cs, O, lines, singles):
    """`singles` off: the ranges are ignored; on: ln 0 = -inf samples, isolated, two in a row and at a range end -- tau of the fused forms
    has NaN exactly where the reference has it and matches elsewhere"""
    nu = R.grid(130)
    data = R.singles_set(nu)
    res, sig, _ = _case(cs, O, lines, nu, [(data, "CO2-CO2")], 10, 3, singles=singles)
    assert bool(np.isnan(sig).any()) == singles
    if singles:
        nn = np.isnan(sig[0])
        assert 0 < nn.sum() < 60 and np.all(np.isnan(sig) == nn[None, :])


# ---- 7: several objects ------------------------------------------------------------------------------------------------------------------

def test_two_pairs_with_different_overlaps(cs, O, lines):
    nu = R.grid(200)
    pairs = [(R.overlap_set(3), "CO2-CO2"), (R.overlap_set(2, "CO2-CH4") + R.band(nu[0], nu[50], 8, R.TS, 7, "CO2-CH4"), "CO2-CH4")]
    res, _, _ = _case(cs, O, lines, nu, pairs, 10, 3)
    assert len(res[0]["col"].U.cia) == 2


def _upload(cs, ctx, slot, data):
    x = cs.CIATables(data)
    bands = [(g, T, z) for g, T, z in x.grids] + [(g, np.array([T]), z) for g, z, T in x.single]
    cs.check(cs.lib().cs_cia_begin(ctx.handle, slot, len(bands)))
    for b, (g, T, z) in enumerate(bands):
        cs.check(cs.lib().cs_cia_band(ctx.handle, slot, b, len(g), cs.dptr(cs.as_f64(g)), len(T), cs.dptr(cs.as_f64(T)), cs.dptr(cs.as_f64(z))))


def _set_cia(cs, ctx, slots, P1, P2, flags=None):
    s = np.array(slots, dtype=np.int32)
    f = np.zeros(len(s), dtype=np.int32) if flags is None else np.array(flags, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    cs.check(cs.lib().cs_column_set_cia(ctx.handle, len(s), ip(s), ip(f), cs.dptr(np.asfortranarray(P1).ravel(order="F").copy()),
                                        cs.dptr(np.asfortranarray(P2).ravel(order="F").copy())))


def _bare_column(cs, lines, ctx, nu, np_, nlob, T=None):
    P = cs.pressuregrid(50.0, 1e5, np_)
    return cs.Column(P, G, _profile(np_) if T is None else T, 0.044, 0.0, 0.0, cs.DirectGas(lines("CO2"), 0.9, nu), core=cs.Discretized(4, nlob),
                     ctx=ctx, _warn=False)


@pytest.mark.parametrize("tune,form", [(SCAN, 3), (CHUNK, 2), (SEP, 0)])
def test_eight_objects_through_the_c_abi(cs, O, lines, tune, form):
    """CS_MAX_CIA = 8 objects in one column, slots and partial pressures given directly to cs_column_set_cia"""
    nu = R.grid(160)
    objs = [R.overlap_set(1 + t % 4) if t < 4 else R.band(nu[10 * t] - 0.01, nu[10 * t + 70], 5 + t, R.TS[t % 3:], 10 + t) for t in range(8)]
    ctx = cs.Context(0)
    try:
        for k, v in tune:
            ctx.set_tuning(k, v)
        for t, d in enumerate(objs):
            _upload(cs, ctx, t, d)
        col = _bare_column(cs, lines, ctx, nu, 10, 3)
        rng = np.random.default_rng(3)
        P1 = col.Pk[None, :] * rng.uniform(0.2, 0.9, (8, col.K))
        P2 = col.Pk[None, :] * rng.uniform(0.2, 0.9, (8, col.K))
        _set_cia(cs, ctx, range(8), P1, P2)
        col.run()
        r = _outputs(col)
        r["sigma"], r["col"] = col.sigma_nodes(), col
        _is(r, form, tune)
        pairs = [(d, "CO2-CO2") for d in objs]
        sig = _sigma_ref(col, pairs, False, False, P1, P2)
        ref = _reference(O, col, sig)
        _above_floor(ref)
        _check(cs, r, sig, ref, sum(objs, []), 3, "8 objects")
        s9 = np.arange(9, dtype=np.int32)
        assert cs.lib().cs_column_set_cia(ctx.handle, 9, s9.ctypes.data_as(C.POINTER(C.c_int)), None, cs.dptr(P1), cs.dptr(P2)) == -1
    finally:
        ctx.close()


# ---- 8: the resident paths -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tune,form", [(SCAN, 3), (CHUNK, 2), (SEP, 0)])
def test_resident_update_set_again_and_reupload(cs, O, lines, tune, form):
    """update(T) to temperatures that move states across band ranges == a fresh column bitwise; cs_column_set_cia again with other partial
    pressures == a fresh column bitwise; a band uploaded again with other samples (another nb) into the same slot, then set again, gives
    the new values, not the cached cells"""
    nu = R.grid(150)
    d1, d2 = R.overlap_set(3), R.band(nu[3], nu[140], 23, R.TS[1:], 4) + R.band(nu[64] - 0.01, nu[100], 3, R.TS, 5)
    np_, nlob = 10, 3
    T2 = _profile(np_, 230.0, 300.0) - 7.0

    def fresh(data, T, P1=None, P2=None):
        c = cs.Context(0)
        try:
            for k, v in tune:
                c.set_tuning(k, v)
            _upload(cs, c, 0, data)
            col = _bare_column(cs, lines, c, nu, np_, nlob, T)
            p1 = col.Pk[None, :] * 0.9 if P1 is None else P1
            _set_cia(cs, c, [0], p1, p1 if P2 is None else P2)
            col.run()
            out = _outputs(col)
            out["sigma"], out["col"] = col.sigma_nodes(), col
            return out
        finally:
            c.close()

    ctx = cs.Context(0)
    try:
        for k, v in tune:
            ctx.set_tuning(k, v)
        col = _column(cs, lines, ctx, nu, [(d1, "CO2-CO2")], np_, nlob)
        col.run()
        a = _outputs(col)
        _is(a, form, tune)
        f0 = fresh(d1, _profile(np_))
        assert np.array_equal(a["tau"], f0["tau"]) and np.array_equal(a["Mup"], f0["Mup"])          # (Python's pairing == the C ABI's inputs)
        col.update(T2)
        col.run()
        b, f1 = _outputs(col), fresh(d1, T2)
        _is(b, form, tune)
        assert not np.array_equal(a["tau"], b["tau"])
        for k in ("tau", "Mup", "Mdn", "Fup", "Fdn"):
            assert np.array_equal(b[k], f1[k]), k
        # other partial pressures, same slot: the per-grid tables are kept
        P1, P2 = col.Pk[None, :] * 0.31, col.Pk[None, :] * 0.77
        slot = ctx.cia_slot(col.U.cia[0].x)
        _set_cia(cs, ctx, [slot], P1, P2)
        col.run()
        c_, f2 = _outputs(col), fresh(d1, T2, P1, P2)
        for k in ("tau", "Mup", "Mdn", "Fup", "Fdn"):
            assert np.array_equal(c_[k], f2[k]), k
        assert not np.array_equal(c_["tau"], b["tau"])
        # other bands in the same slot
        _upload(cs, ctx, slot, d2)
        _set_cia(cs, ctx, [slot], P1, P2)
        col.run()
        d_ = _outputs(col)
        d_["sigma"], d_["col"] = col.sigma_nodes(), col
        sig = _sigma_ref(col, [(d2, "CO2-CO2")], False, False, P1, P2)
        _is(d_, form, tune)
        ref = _reference(O, col, sig)
        _above_floor(ref)
        _check(cs, d_, sig, ref, d2, nlob, "re-uploaded")
        f3 = fresh(d2, T2, P1, P2)
        for k in ("tau", "Mup", "Mdn"):
            assert np.array_equal(d_[k], f3[k]), k
    finally:
        ctx.close()


# ---- 9: batches -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,extrap", [("overlap4", False), ("temperatures", True), ("temperatures", False)])
def test_run_batch(cs, O, lines, which, extrap):
    """cs_column_batch evaluates the pairs at B K = 76 states through its own code (cia_states over B K, the unfused k_cia): per
    profile against the reference.  A batch returns band fluxes only, so they are what is compared (1e-11 of the largest); every profile
    must have a good share of its layers above the optical-depth floor, or the fluxes would not depend on the bands"""
    nu = R.grid(200)
    data = R.overlap_set(4) if which == "overlap4" else R.overlap_set(3) + R.band(nu[0] + 0.01, nu[40], 6, (200.0, 300.0), 9)
    np_, nlob = 10, 3
    ctx = cs.Context(0)
    try:
        col = _column(cs, lines, ctx, nu, [(data, "CO2-CO2")], np_, nlob, extrap=extrap)
        Ts = [_profile(np_), _profile(np_, 230.0, 300.0) - 7.0, _profile(np_, 150.0, 400.0), np.full(np_, 260.0) + np.arange(np_)]
        assert len(Ts) * col.K > 64
        Fup, Fdn = col.run_batch(Ts)
        for b, T in enumerate(Ts):
            fT = cs.core.formprofile(col.P, T)
            Tn, mun = cs.core.lobattoevaluations(col.P, fT, col._fmu, nlob)
            Tk = cs.core.nodevalues(Tn, nlob)
            sig = _sigma_ref(col, [(data, "CO2-CO2")], extrap, False, Tk=Tk)
            ref = O.fluxes_discretized(col.nu, col.P, col.g, nlob, Tn, mun, np.array([fT(p) for p in col.P]), [col.gases[0].sl], ["voigt"], [25.0],
                                       col.conc, sigma_extra=sig, nstream=col.core.nstream, theta_s=col.theta_s)
            _above_floor(ref)
            e = max(np.max(np.abs(Fup[b] - ref["Fup"])), np.max(np.abs(Fdn[b] - ref["Fdn"]))) / ref["Fup"].max()
            print(f"  profile {b}: flux err {e:.2e}")
            assert e < 1e-11, (b, e)
    finally:
        ctx.close()
