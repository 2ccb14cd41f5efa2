"""40-digit reference of the column's slant optical depth and of its per-tile transmittances to space (k_depth, cs_kernels.h: the
CS_TAU_TOTAL and CS_TAU_TILES modes of a resident column) from a cross-section plane, with a first-order forward-error bound per
element, and a plain double restatement that can carry one planted defect.  In the style of tests/flux_ref.py, whose constants, planes
and helpers it uses; tests/test_depth_ref.py (host) and tests/test_gpu_depth_modes.py (device) use it.  Everything is mpmath on the
doubles the implementation is given; no oracle, no GPU.

Restated from the reference's core/discretized.jl (dDepth, :92-134 -- no floor) and fluxes.jl:68-109 (opticaldepth, transmittance):
  beta_k  = C (sigma_k / mu_k), C = 1e-4 Na / g
  tau_i   = sum_n (dP_i ws_n) beta_{i (nlob - 1) + n}            the sum layer_depth forms before its floor
  m       = 1 / cos(theta_s)
  D_0 = 0, D_{i+1} = D_i + tau_i m                               level by level from the top; D = D_{np-1}
  T[i, t] = sum over the points j of tile t of w_j exp(-D_i(nu_j))      tiles of 64 points, the last one ragged; row 0 is sum w_j
The Lobatto weights ws and the weights w are arguments, taken as exact, as in flux_ref.

The bound (`bounds`), to first order in u = 2^-53; each term is a count of the roundings k_depth performs (a fused multiply-add only
removes one; the numpy restatement performs the same operations without contraction):
  D      a layer sum: flux_ref's count for layer_depth, (nlob + 7) u -- node_beta: sigma / mu, C x (2), C = 1e-4 Na / g in double (3);
         dP (1), dP ws_n (1), the product with beta (1), nlob - 1 additions of positive terms.  m: cos(theta_s) on the host (1 ulp = 2 u),
         the correctly rounded division (1), the product tau_i m (1): 4 u.  The accumulation: one addition per layer, each u of a
         partial sum that is at most the total (positive terms): at level i, i u -- counted nl u at every level.
         |D_i - exact| <= (nlob + nl + 11) u D_i.  D_0 = 0 is exact.
  term   w_j exp(-D): through D, exp(-D) D rel_D (the conditioning of the exponential on its argument); the exponential's own error
         E u exp(-D), E = flux_ref.E_EXP["libm"] = 2 -- k_depth calls the library's exp (1 ulp in HIP's table of math functions), numpy
         calls libm's: e_term = w_j exp(-D) (D rel_D + E u).
  sum    the product w_j exp(-D) (1) and the 63 additions of the wave sum in whatever order the reduction takes, all terms >= 0: counted
         66 u sum_j |term_j|, as tests/test_gpu_reduced_spectra.py counts the same sum of the tiles mode of the fluxes.
  underflow  a result below the normal range is rounded absolutely, 2^-1074 per operation: per term the exponential, the product and
         the addition, 3 x 64 per tile; D: the products and sums of nl layers, (3 nlob + 2) nl.  It matters only where exp(-D) leaves
         the normal range (D > 708).
Nothing is fitted: tests/test_depth_ref.py holds the numpy restatement to the bound at factor 1, requires the bound to reject every
planted fault, and to stay below 1e-13 of the value wherever the exponential's conditioning allows that at all (see there).
"""
import math

import numpy as np
from mpmath import mp, mpf

import flux_ref as F

U = F.U
TILE = 64
E = F.E_EXP["libm"]

_exp_neg_arr = np.frompyfunc(F._exp_neg, 1, 1)


def tile_ranges(nnu):
    return [(j0, min(j0 + TILE, nnu)) for j0 in range(0, nnu, TILE)]


def case(cs, nlob=3, np_=9, nnu=F.NNU_GPU, theta=0.6, sset=None):
    """flux_ref.case's column (profile (a), its mu(T, P), the plane sigma_plane(K, nnu, sset)) as the doubles an implementation is given,
    which also takes np = 2: one layer from 5 Pa to the surface (pressuregrid starts at three levels)"""
    P = cs.pressuregrid(5.0, 1e5, np_) if np_ > 2 else np.array([5.0, 1e5])
    T = F.profile("a", P)
    Tn, mun = cs.core.lobattoevaluations(P, cs.core.formprofile(P, T), F.fmu, nlob)
    K = (np_ - 1) * (nlob - 1) + 1
    nu = np.linspace(F.NU_LO, F.NU_HI, nnu)
    return dict(nu=nu, P=P, g=F.G, T=T, muk=cs.core.nodevalues(mun, nlob), K=K, nlob=nlob, theta_s=theta,
                sigma=F.sigma_plane(K, nnu, F.S_FULL if sset is None else sset), ws=cs.lobattonodes(nlob)[1], Pk=cs.core.nodepressures(P, nlob))


def mp_depth(P, g, muk, sigma, theta_s, ws, wts=None, dps=40):
    """dict(D=[np, nnu] cumulative slant depths (row np-1: the column's), T=[np, ntile] tile sums or None, absT = the same sums of
    w_j exp(-D) D (what the conditioning term needs)) as object arrays of mpf.  sigma: [K, nnu] doubles, node k = i (nlob - 1) + n"""
    with mp.workdps(dps):
        sigma = np.asarray(sigma, float)
        nlob, np_, nl, nnu = len(ws), len(P), len(P) - 1, sigma.shape[1]
        assert sigma.shape[0] == nl * (nlob - 1) + 1 == len(muk)
        ws_ = [mpf(float(x)) for x in ws]
        C = mpf("1e-4") * mpf(F.NA_) / mpf(float(g))
        Pm = [mpf(float(p)) for p in P]
        mu_ = F._mpf_arr(np.asarray(muk, float))
        beta = C * (F._mpf_arr(sigma) / mu_[:, None])
        m = 1 / mp.cos(mpf(float(theta_s)))
        D = np.empty((np_, nnu), object)
        D[0] = mpf(0)
        for i in range(nl):
            ti = np.full(nnu, mpf(0), object)
            for n in range(nlob):
                ti = ti + ((Pm[i + 1] - Pm[i]) * ws_[n]) * beta[i * (nlob - 1) + n]
            D[i + 1] = D[i] + ti * m
        T = DT = None
        if wts is not None:
            w = F._mpf_arr(np.asarray(wts, float))
            rng = tile_ranges(nnu)
            T, DT = np.empty((np_, len(rng)), object), np.empty((np_, len(rng)), object)
            for i in range(np_):
                term = w * _exp_neg_arr(D[i])
                for t, (j0, j1) in enumerate(rng):
                    T[i, t] = mp.fsum(term[j0:j1])
                    DT[i, t] = mp.fsum(term[j0:j1] * D[i, j0:j1])
        return dict(D=D, T=T, DT=DT, nlob=nlob, nl=nl)


def bounds(ref):
    """dict(D=[np, nnu], T=[np, ntile]) of doubles: |computed - exact| <= bound (the docstring's count).  The weights may have either
    sign in principle (trapezoid weights are positive): absolute values throughout"""
    nlob, nl = ref["nlob"], ref["nl"]
    rel_D = (nlob + nl + 11) * U
    tiny = 2.0 ** -1074
    D = np.abs(F.to_float(ref["D"]))
    out = dict(D=rel_D * D + (3 * nlob + 2) * nl * tiny, T=None, rel_D=rel_D)
    out["D"][0] = 0.0
    if ref["T"] is not None:
        T, DT = np.abs(F.to_float(ref["T"])), np.abs(F.to_float(ref["DT"]))
        out["T"] = DT * rel_D + T * (E * U) + 66 * U * T + 3 * TILE * tiny
    return out


FAULTS = ("floor", "last_layer", "end_node", "m", "weights", "tile_edge")


def np_depth(P, g, muk, sigma, theta_s, ws, wts, fault=None):
    """the same in plain numpy doubles: dict(D=[np, nnu], T=[np, ntile]).  fault (one at a time):
      "floor"       dDepth!'s floor max(tau_i, 1e-6) applied to every layer
      "last_layer"  the last layer left out of the accumulation
      "end_node"    a layer's end node not shared: layer i > 0 starts one node late (its first node is the node after the end node of
                    layer i - 1, its last the column's last at most)
      "m"           the slant factor left out
      "weights"     the tile sums without the weights
      "tile_edge"   every tile boundary one point late: tile t = points [64 t + 1, 64 t + 65) (tile 0 from point 0)"""
    assert fault is None or fault in FAULTS
    P, muk, sigma, wts = (np.asarray(a, float) for a in (P, muk, sigma, wts))
    ws = np.array([float(x) for x in ws])
    nlob, np_, nl, (K, nnu) = len(ws), len(P), len(P) - 1, sigma.shape
    C = 1e-4 * F.NA_ / g
    beta = C * (sigma / muk[:, None])
    m = 1.0 if fault == "m" else 1.0 / math.cos(theta_s)
    D = np.zeros((np_, nnu))
    for i in range(nl):
        dP = P[i + 1] - P[i]
        ti = np.zeros(nnu)
        k0 = i * (nlob - 1) + (1 if fault == "end_node" and i > 0 else 0)
        for n in range(nlob):
            ti = ti + (dP * ws[n]) * beta[min(k0 + n, K - 1)]
        if fault == "floor":
            ti = np.maximum(ti, 1e-6)
        D[i + 1] = D[i] if (fault == "last_layer" and i == nl - 1) else D[i] + ti * m
    rng = tile_ranges(nnu)
    if fault == "tile_edge":
        rng = [(j0 + (1 if j0 else 0), min(j1 + 1, nnu)) for j0, j1 in rng]
    T = np.zeros((np_, len(rng)))
    with np.errstate(under="ignore"):
        term = np.exp(-D) * (1.0 if fault == "weights" else wts[None, :])
    for t, (j0, j1) in enumerate(rng):
        T[:, t] = np.sum(term[:, j0:j1], axis=1)
    return dict(D=D, T=T)


def ratios(got, ref, bnd):
    """worst |got - ref| / bound of D and of T (flux_ref.ratio: 40-digit differences, never NaN)"""
    return {k: F.ratio(got[k], ref[k], bnd[k]) for k in ("D", "T") if got.get(k) is not None and ref.get(k) is not None}


def host_formula(P, g, muk, sigma, theta, ws):
    """opticaldepth as the package formed it on the host before k_depth existed, on a fetched plane [K, nnu] (the last row of
    np_depth's D, operation for operation)"""
    return np_depth(P, g, muk, sigma, theta, ws, np.ones(np.shape(sigma)[1]))["D"][-1]
