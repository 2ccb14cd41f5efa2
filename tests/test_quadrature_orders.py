"""CPU tests: the quadratures at every order the C ABI accepts (nstream 1..16, nlobatto 2..16) against 50-digit mpmath, and the oracle's
flux stage at high orders against a 30-digit restatement of the reference's formulas.

The GPU tests of the high orders (test_gpu_flux_orders.py) compare the device with the oracle; until now the oracle had been compared
with itself there (the quadrature goldens pin Lobatto n = 2..5 and streams n = 1, 2, 3, 5, 8, 16).  Both are anchored here:
  - Gauss-Legendre mapped to the hemisphere, core/shared.jl:4-21 (streamnodes), and Gauss-Lobatto on [0, 1], core/discretized.jl:2-9
    (lobattonodes), from the roots of the explicit Legendre coefficients (mp.polyroots);
  - dDepth! (discretized.jl:136-177), layerplanck (:85-87) and the two sweeps of dMonoflux! (:258-330) for one column of a gray term and a
    wavenumber-dependent extra term whose layer optical depths run from the 1e-6 floor to ~50, with a stellar beam and an albedo.
"""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

from flux_ref import mp_fluxes, to_float


def _legendre_coeffs(n):
    """P_n as integer-free mpf coefficients, lowest degree first (Bonnet's recurrence)"""
    p0, p1 = [mpf(1)], [mpf(0), mpf(1)]
    if n == 0:
        return p0
    for j in range(1, n):
        p2 = [mpf(0)] * (j + 2)
        for i, c in enumerate(p1):
            p2[i + 1] += (2 * j + 1) * c / (j + 1)
        for i, c in enumerate(p0):
            p2[i] -= j * c / (j + 1)
        p0, p1 = p1, p2
    return p1


def _peval(c, x):
    return mp.polyval(c[::-1], x)


def _deriv(c):
    return [i * c[i] for i in range(1, len(c))]


def _roots(c):
    if len(c) == 1:
        return []
    r = mp.polyroots(c[::-1], maxsteps=400, extraprec=400)
    return sorted(mp.re(z) for z in r)


def _mp_streamnodes(n):
    with mp.workdps(50):
        c = _legendre_coeffs(n)
        dc = _deriv(c)
        x = _roots(c)
        w = [2 / ((1 - z * z) * _peval(dc, z) ** 2) for z in x]
        m, W = [], []
        for xi, wi in zip(x, w):
            th = (mp.pi / 2) * (xi + 1) / 2
            m.append(1 / mp.cos(th))
            W.append(2 * mp.pi * ((mp.pi / 2) * wi / 2) * mp.cos(th) * mp.sin(th))
        return m, W


def _mp_lobattonodes(n):
    with mp.workdps(50):
        N = n - 1
        c = _legendre_coeffs(N)
        x = [mpf(-1)] + _roots(_deriv(c)) + [mpf(1)]
        w = [mpf(2) / (N * (N + 1) * _peval(c, z) ** 2) for z in x]
        return [(z + 1) / 2 for z in x], [v / 2 for v in w]


_STREAMS = {n: _mp_streamnodes(n) for n in range(1, 17)}
_LOBATTO = {n: _mp_lobattonodes(n) for n in range(2, 17)}


def _rel(a, ref):
    return max(float(abs((mpf(float(x)) - r) / r)) for x, r in zip(a, ref))


def _abs(a, ref):
    return max(float(abs(mpf(float(x)) - r)) for x, r in zip(a, ref))


@pytest.mark.parametrize("n", range(1, 17))
def test_streamnodes_every_order(cs, O, n):
    """library and oracle at every stream count: 1e-13 relative (measured <= 2.4e-14, most of it 1/cos near pi/2)"""
    m_ref, W_ref = _STREAMS[n]
    for m, W in (cs.streamnodes(n), O.streamnodes(n)):
        assert len(m) == n
        assert _rel(m, m_ref) < 1e-13 and _rel(W, W_ref) < 1e-13, n


@pytest.mark.parametrize("n", range(2, 17))
def test_lobattonodes_every_order(cs, O, n):
    """library and oracle at every Lobatto order: nodes and weights to 1e-15 absolute (measured <= 1e-16), weights summing to one, nodes
    symmetric about 1/2, end nodes exactly 0 and 1"""
    x_ref, w_ref = _LOBATTO[n]
    for x, w in (cs.lobattonodes(n), O.lobattonodes(n)):
        assert len(x) == n
        assert _abs(x, x_ref) < 1e-15 and _abs(w, w_ref) < 1e-15, n
        assert abs(math.fsum(w) - 1.0) <= 2.0 ** -51      # (measured: 2^-51 at n = 14, exact sum of the rounded weights)
        assert np.max(np.abs(x + x[::-1] - 1.0)) < 1e-16
        assert x[0] == 0.0 and x[-1] == 1.0


def test_orders_outside_the_abi_refused(cs):
    for n in (0, 17):
        with pytest.raises(cs.ClearSkyHIPError):
            cs.streamnodes(n)
    for n in (1, 17):
        with pytest.raises(cs.ClearSkyHIPError):
            cs.lobattonodes(n)


# ---- the oracle's flux stage, restated ----------------------------------------------------------------------------------------

NU = np.array([150.0, 420.0, 667.0, 905.5, 1200.0, 1610.0, 2300.0, 3050.0])      # 8 wavenumbers [cm^-1]
P = np.array([2.0, 300.0, 3000.0, 15000.0, 40000.0, 70000.0, 1e5])               # 6 layers, ascending [Pa]
G, THETA_S, SIGMA_GRAY = 9.8, 0.5, 3e-31
S_TOA = np.array([0.0, 0.3, 1.2, 0.0, 2.5, 0.8, 0.05, 0.4])
ALBEDO = np.array([0.0, 0.1, 0.35, 0.6, 0.2, 0.9, 0.05, 0.3])


def _column(nlob):
    """node temperatures / molar masses [nlob, nl] (column-major as the ABI takes them), level temperatures, and the extra cross-section
    [K, nnu]: ~6e-32 .. 6e-24 cm^2 across the grid, modulated along the column so that every Lobatto node weighs in"""
    nl = len(P) - 1
    xs = np.asarray(_LOBATTO[nlob][0], dtype=float)
    Tn = np.zeros((nlob, nl), order="F")
    mun = np.zeros((nlob, nl), order="F")
    for i in range(nl):
        for n in range(nlob):
            p = P[i] + (P[i + 1] - P[i]) * xs[n]
            Tn[n, i] = 200.0 + 90.0 * (p / 1e5) ** 0.19
            mun[n, i] = 0.029 - 0.002 * (p / 1e5)
    Tlev = 200.0 + 90.0 * (P / 1e5) ** 0.19
    K = nl * (nlob - 1) + 1
    scale = 6e-24 * 10.0 ** np.linspace(-8.0, 0.0, len(NU))
    k = np.arange(K)[:, None]
    extra = scale[None, :] * (1.0 + 0.5 * np.sin(0.7 * k + NU[None, :] / 300.0))
    return Tn, mun, Tlev, extra


def _mp_fluxes(nstream, nlob, Tn, mun, Tlev, extra):
    """dDepth!, layerplanck and dMonoflux! of discretized.jl in 30-digit arithmetic on the same double inputs (flux_ref.mp_fluxes with
    the 50-digit quadrature numbers and the exact sum of the gray and the extra term); band fluxes by the trapezoid rule (util.jl:26-33)"""
    with mp.workdps(30):
        sigma = np.empty(extra.shape, dtype=object)
        for k in range(extra.shape[0]):
            for j in range(extra.shape[1]):
                sigma[k, j] = mpf(SIGMA_GRAY) + mpf(float(extra[k, j]))
        ws, (m, W) = _LOBATTO[nlob][1], _STREAMS[nstream]
        # node k = i (nlob - 1) + n: node 0 of a layer is the last node of the layer above (the top level: mun[0, 0])
        muk = [mun[0, 0]] + [mun[n, i] for i in range(mun.shape[1]) for n in range(1, nlob)]
        r = mp_fluxes(NU, P, G, muk, Tlev, sigma, S_TOA, ALBEDO, THETA_S, ws, m, W, dps=30)
        Mu_mp, Md_mp = r["Mup"].T, r["Mdn"].T                  # [nnu][np]
        nnu, np_ = len(NU), len(P)
        nuv = [mpf(float(v)) for v in NU]
        trapz = lambda M: [float(mp.fsum((nuv[j + 1] - nuv[j]) * (M[j][i] + M[j + 1][i]) / 2 for j in range(nnu - 1))) for i in range(np_)]
        return dict(tau=to_float(r["tau"]), Mup=to_float(r["Mup"]), Mdn=to_float(r["Mdn"]), Fup=np.array(trapz(Mu_mp)),
                    Fdn=np.array(trapz(Md_mp)))


def _source_rounding(nstream, Tlev, tau):
    """per wavenumber: how far M+- of double arithmetic may stray from exact arithmetic through exp(-tau m) alone.  layerplanck's
    (1 - t)(B1 - B2) / (tau m) turns the rounding of t (1 ulp below 1: 2^-53) into 2^-53 / (tau m) |B1 - B2| -- 1e-10 |dB| at the 1e-6
    floor -- per layer and stream, weighted by W_k and carried by transmissivities <= 1; twice that (conftest.source_rounding_bound is
    the same bound as one number for the whole grid)"""
    m, W = (np.array([float(v) for v in a]) for a in _STREAMS[nstream])
    B = np.array([[float(x) for x in row] for row in _planck_mp(Tlev)])
    return 2 * 2.0 ** -53 * np.sum(W / m) * np.sum(np.abs(np.diff(B, axis=0)) / tau, axis=0)


def _planck_mp(Tlev):
    with mp.workdps(30):
        h, c, kB = mpf(6.62607015e-34), mpf(299792458.0), mpf(1.38064852e-23)
        return [[100 * 2 * h * c ** 2 * (100 * mpf(float(v))) ** 3 / (mp.exp(h * c * 100 * mpf(float(v)) / (kB * mpf(float(T)))) - 1)
                 for v in NU] for T in Tlev]


@pytest.mark.parametrize("nlob", [2, 4, 6, 11, 16])
@pytest.mark.parametrize("nstream", [1, 2, 7, 9, 16])
def test_oracle_flux_stage_high_orders(O, nstream, nlob):
    """O.fluxes_discretized (gray + extra term only: no line shapes) against the 30-digit restatement: tau to 1e-13 relative, M+- and
    F+- to 1e-13 of their maximum plus, per wavenumber, the rounding of exp(-tau m) in double that (1 - t) / tau carries near the 1e-6
    floor (_source_rounding: measured at most a tenth of it; the wavenumbers of tau >= 0.05 agree to 5e-15 of the maximum)"""
    Tn, mun, Tlev, extra = _column(nlob)
    r = O.fluxes_discretized(NU, P, G, nlob, Tn, mun, Tlev, [], [], [], np.zeros((0, extra.shape[0])), sigma_gray=SIGMA_GRAY,
                             sigma_extra=extra, S_toa=S_TOA, albedo=ALBEDO, theta_s=THETA_S, nstream=nstream)
    ref = _mp_fluxes(nstream, nlob, Tn, mun, Tlev, extra)
    assert ref["tau"].min() == 1e-6 and 20.0 < ref["tau"].max() < 100.0        # the column spans the floor to ~50
    assert np.max(np.abs(r["tau"] - ref["tau"]) / ref["tau"]) < 1e-13
    amp = _source_rounding(nstream, Tlev, ref["tau"])
    for k in ("Mup", "Mdn"):
        sm = np.max(np.abs(ref[k]))
        assert np.all(np.abs(r[k] - ref[k]) < 1e-13 * sm + amp[None, :]), k
    wts = np.zeros(len(NU))
    wts[:-1] += np.diff(NU) / 2
    wts[1:] += np.diff(NU) / 2
    for k in ("Fup", "Fdn"):
        assert np.max(np.abs(r[k] - ref[k])) < 1e-13 * np.max(np.abs(ref[k])) + np.sum(wts * amp), k
