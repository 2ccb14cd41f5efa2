"""40-digit reference of the flux stage -- dDepth!, Planck, layerplanck, the two sweeps, the stellar beam, the surface -- with a
first-order forward-error bound per output element, a plain double restatement that can carry one planted defect, and the inputs the
tests share.  tests/test_flux_ref.py (host: the oracle, the planted faults, sharpness) and tests/test_gpu_flux_ref.py (every device form)
use it; tests/test_quadrature_orders.py takes its 30-digit restatement from here.  Everything is mpmath on the doubles the
implementation is given; no oracle, no GPU.

Restated from the reference's core/discretized.jl (as csrc/cs_kernels.h and oracle/cs_oracle.c restate it):
  beta_k   = C (sigma_k / mu_k), C = 1e-4 Na / g                                     :76-81, fluxes.jl:259
  tau_i    = max(sum_n (dP_i ws_n) beta_{i (nlob - 1) + n}, 1e-6)                     dDepth! :136-177
  B        = 100 (2 h c^2 num^3) / (exp(h c num / (k T)) - 1), num = 100 nu           radiation.jl:48-54
  Be       = B2 (1 - t) - (B1 - B2) t + (1 - t)(B1 - B2) / (tau m_k), t = exp(-tau m_k)      layerplanck :85-87
  I <- I t + Be per stream and layer; M-[i + 1] = sum_k W_k I_k + c fS prod exp(-tau / c), c = cos theta_s       :282-304
  Is = M-[np] fa / pi + B[np]; M+[np] = pi Is; upward the same recurrence from Is     :309-322
The quadrature numbers (Lobatto weights ws, stream secants m and weights W) are arguments: the tests hand over the doubles the
implementation under test uses (cs.lobattonodes / cs.streamnodes for the device, O.* for the oracle) and they are taken as exact
rationals -- how good they are is tests/test_quadrature_orders.py's business.  h, c, k, Na are the doubles of the sources.
One convention is the implementations', not mathematics: where exp(h c num / k T) overflows a double (argument, formed in double as the
sources form it, above ln DBL_MAX), B is the 0 that 100 p / inf gives.

The bound (`bounds`): |computed - exact| <= bound, element by element, to first order in u = 2^-53.  Every quantity of the recurrences
carries an absolute error beside its value; each term below is the count of roundings of the named function of cs_kernels.h (the
oracle's C performs the same operations without contraction; a fused multiply-add only removes a rounding).  Division and sqrt of
doubles are correctly rounded on both sides (hipcc -O3 and gcc -O3, no fast-math flag: _lib.py, oracle/oracle.py).
  E      the exponential's error in units of u.  "libm": 2 (glibc documents exp at 1 ulp = 2 u).  "device": 6 -- exp_rt is asserted
         within 2 ulp of libm (tests/test_gpu_kat.py::test_exp_rt_vs_libm), so 3 ulp of the true value.  That test covers
         [-1000, 20], which holds every transmissivity; planck calls exp_rt at positive arguments up to ln DBL_MAX = 709.8, where no
         test of the project asserts the figure yet.  exp_rt's reduction and polynomial are the same on both sides of 0 (|r| <= ln 2 / 2,
         n ln2_hi exact for |n| < 2^11), so the figure is used there too, and tests/test_gpu_flux_ref.py::test_planck_regimes, which
         runs x from 5e-6 to overflow, is then the check of it.  The stellar beam's exp(-t / c) is the library's exp on both sides
         (1 ulp in glibc's and in HIP's tables of math functions): 2 for either arithmetic.
  Ecos   cos(theta_s) on the host: 1 ulp = 2 u.
  tau    node_beta: sigma / mu, C x (2), C itself = 1e-4 Na / g in double (3: the constant, a product, a division); layer_depth:
         dP (1), dP ws_n (1), the product with beta (1), nlob - 1 additions of positive terms: rel_tau = (nlob + 7) u.  A layer whose
         exact depth is below the floor by more than that is exactly 1e-6 on both sides (error 0).
  B      planck: num (1) enters x once and p three times; x = (h c) num / (k T): 4 more = 5; p = 2 h (c c) num^3: 5 + 3 = 8; 100 p (1),
         the division (1), exp(x) - 1: the subtraction (1) and, relative to exp(x) - 1, exp(x) / (exp(x) - 1) (5 x u + E u):
         rel_B = [11 + (5 x + E) / (1 - e^-x)] u -- E / x at small x (test_gpu_kat's 4 2^-52 / min(x, 1) is this term for the pair of
         exponentials it compares), 5 x u in the Wien tail (the conditioning of exp on its rounded argument).
  t      stream_tr: a = tau m_k rounded (rel_tau + u), t = exp(-a): e_t = t [a (rel_tau + u) + E u] (+ underflow, below): the
         conditioning of exp(-tau m) and the exponential's own error.
  1/(tau m)   the device forms (1 / tau)(1 / m_k): a division, the stored 1 / m_k (1), the product (1): rel_q = rel_tau + 3 u; the
         oracle divides by the rounded tau m_k: rel_tau + 2 u.
  Be     layerplanck_inv, with s = 1 - t, dB = B1 - B2, q = 1 / (tau m), g = s q - t (0 <= g <= s):
           through t (the same rounded t multiplies I in stream_step, so the two sensitivities are taken together):
                         |I - B1 - dB q| e_t       -- the cancellation term: u / (tau m) |B1 - B2| per unit of e_t near t = 1
           rounding of s: u s |B2 + dB q|          -- again |dB| u, the second cancellation term
           through B1:   g e_B1;  through B2: (s - g) e_B2;  rounding of dB: g u |dB|   (dB enters as -dB t + s dB q = g dB: an
                         isothermal layer, whose two Planck values are the same double, has dB = 0 exactly and loses these terms)
           through q:    |s dB q| rel_q
           its own products and sums: u (|B2 s| + |dB t| + 2 |s dB q| + |B2 s - dB t| + |Be|)
  I      stream_step: I' = I t + Be: e_I' = e_I t + (terms above) + u (|I t| + |I'|): propagation with t <= 1.
  M      sweep_step: sum_k W_k I_k: sum_k W_k e_Ik + NS u sum_k W_k |I_k| (a product and at most NS - 1 additions each).
  beam   Ms0 = c fS: (Ecos + u) Ms0; per layer exp(-tau / c): e = ts [(tau / c)(rel_tau + Ecos + u) + 2 u]; the product (1); the sum
         M + Ms (1).
  surface  surface_intensity: Md fa / pi + Bs: e_Md fa / pi + 3 u |Md fa / pi| (product, division, pi as a double: 0.35 u, counted 1)
         + e_Bs + u |Is|; M+[np] = Is pi: pi e_Is + 2 u pi Is.
  scan   k_flux_scan forms the intensity entering the next chunk as X' = X A + B_chunk with A the product of the chunk's `per`
         transmissivities and B_chunk the chunk run from zero.  X A + B_chunk is the same function of the rounded t's as the layer by
         layer recurrence (it is linear), so its sensitivities are those above; its own roundings are A's products (per - 1), the
         chunk from zero (never more than the chunk from X >= 0) and the final multiply-add (2): at every chunk boundary
         e_X += u (per A X + 2 X').  The beam's Ms A_s likewise: per u Ms'.  `bounds(..., per=)` adds them; per = layers per wave,
         read from flux_plan (scan_per below).
  underflow  a result below the normal range is rounded absolutely: 2^-1074 per operation.  Operations that can reach an element:
         per (stream, layer) 15 -- stream_tr (product, exp), sweep_step's 1/(tau m) product, layerplanck_inv (1 - t, B1 - B2, four
         products, two sums), stream_step (product, sum), W_k I_k and its addition -- in two sweeps (M+ sees the downward one through
         the albedo): 30 NS nl; planck 10 per level, the beam 3 per layer (division, exp, product), the surface 4:
         TINY = (30 NS nl + 13 nl + 14) 2^-1074, ~1e-320.  It matters only where a product of a Wien-tail Planck value and a
         transmissivity leaves the normal range.
Nothing here is fitted to an implementation: tests/test_flux_ref.py holds the oracle to bounds("libm") at factor 1 (so no term is
missing) and requires the bound to reject every planted fault and to stay below 1e-13 / 1e-12 of the value (so no term is idle).
"""
import math

import numpy as np
from mpmath import mp, mpf

U = 2.0 ** -53
E_EXP = {"libm": 2.0, "device": 6.0}
E_COS = 2.0
E_BEAM = 2.0                               # the library exp of the stellar beam, 1 ulp on either side
LN_DBL_MAX = 709.782712893384
H_, C_, KB_, NA_ = 6.62607015e-34, 299792458.0, 1.38064852e-23, 6.02214076e23
D = 24                                     # period of the cross-section plane along the grid
NNU_GPU = 64 * 2 + 17                      # three tiles, a ragged last one
G = 9.8

_mpf_arr = np.frompyfunc(lambda x: mpf(x), 1, 1)
_flt_arr = np.frompyfunc(float, 1, 1)


def to_float(a):
    return _flt_arr(a).astype(float)


# ---- the 40-digit reference -----------------------------------------------------------------------------------------------------

_EXP = {}


def _exp_neg(a):
    """exp(-a), memoised on its argument (and the working precision): the inputs repeat optical-depth columns on purpose"""
    key = (mp.prec, a)
    v = _EXP.get(key)
    if v is None:
        if len(_EXP) > 400000:
            _EXP.clear()
        v = _EXP[key] = mp.exp(-a)
    return v


def planck_x_double(nu, T):
    """the exponential's argument as the sources form it in double (radiation.jl:48-54)"""
    return H_ * C_ * (100.0 * nu) / (KB_ * T)


def mp_fluxes(nu, P, g, muk, Tlev, sigma, S_toa, albedo, theta_s, ws, m, W, dps=40, detail=False):
    """tau [nl, nnu], M+ and M- [np, nnu] as object arrays of mpf.  sigma: [K, nnu] of doubles (or mpf), node k = i (nlob - 1) + n;
    S_toa, albedo: [nnu] or None; ws, m, W: the quadrature numbers, taken as exact.  detail: also the double copies of the
    intermediates that `bounds` needs"""
    with mp.workdps(dps):
        nlob, ns, np_, nl, nnu = len(ws), len(m), len(P), len(P) - 1, len(nu)
        ws_, m_, W_ = [mpf(x) for x in ws], [mpf(x) for x in m], [mpf(x) for x in W]
        h, c, kB, Na = mpf(H_), mpf(C_), mpf(KB_), mpf(NA_)
        C = mpf("1e-4") * Na / mpf(g)
        Pm = [mpf(float(p)) for p in P]
        dPw = [[(Pm[i + 1] - Pm[i]) * ws_[n] for n in range(nlob)] for i in range(nl)]
        mu_ = [mpf(x) for x in muk]
        cth = mp.cos(mpf(theta_s))
        floor = mpf(1e-6)                          # the double the sources compare with
        zero, one = mpf(0), mpf(1)
        obj = lambda *s: np.empty(s, dtype=object)
        tau, Mu, Md = obj(nl, nnu), obj(np_, nnu), obj(np_, nnu)
        if detail:
            f = lambda *s: np.zeros(s)
            d = dict(B=f(np_, nnu), x=f(np_, nnu), tau_raw=f(nl, nnu), t=f(ns, nl, nnu), s=f(ns, nl, nnu), q=f(ns, nl, nnu),
                     g=f(ns, nl, nnu), Id=f(ns, np_, nnu), Iu=f(ns, np_, nnu), Ms=f(np_, nnu), ts=f(nl, nnu), Is=f(nnu))
        cols = {}                                      # per optical-depth column: tau and, per stream and layer, (t, s, q, g)
        for j in range(nnu):
            v = float(nu[j])
            num = 100 * mpf(v)
            B = []
            for i, T in enumerate(Tlev):
                xd = planck_x_double(v, float(T))
                if xd > LN_DBL_MAX:
                    B.append(zero)                     # 100 p / inf
                else:
                    B.append(100 * 2 * h * c ** 2 * num ** 3 / (mp.exp(h * c * num / (kB * mpf(float(T)))) - 1))
                if detail:
                    d["x"][i, j] = xd
            key = tuple(sigma[:, j])
            col = cols.get(key)
            if col is None:
                beta = [C * (mpf(sigma[k, j]) / mu_[k]) for k in range(len(mu_))]
                traw = [mp.fsum(dPw[i][n] * beta[i * (nlob - 1) + n] for n in range(nlob)) for i in range(nl)]
                t = [max(x, floor) for x in traw]
                per = []
                for k in range(ns):
                    row = []
                    for i in range(nl):
                        a = t[i] * m_[k]
                        tr = _exp_neg(a)
                        s, q = one - tr, one / a
                        row.append((tr, s, q, s * q - tr))
                    per.append(row)
                ts = [_exp_neg(x / cth) for x in t]
                col = cols[key] = (traw, t, per, ts)
            traw, t, per, ts = col
            tau[:, j] = t
            md, mu = [zero] * np_, [zero] * np_
            for k in range(ns):
                I, row = zero, per[k]
                for i in range(nl):
                    tr, s, q, _ = row[i]
                    dB = B[i] - B[i + 1]
                    I = I * tr + (B[i + 1] * s - dB * tr + s * dB * q)
                    md[i + 1] += W_[k] * I
                    if detail:
                        d["Id"][k, i + 1, j] = I
            Ms = cth * mpf(float(S_toa[j])) if S_toa is not None else zero
            md[0] += Ms
            if detail:
                d["Ms"][0, j] = Ms
            for i in range(nl):
                Ms = Ms * ts[i]
                md[i + 1] += Ms
                if detail:
                    d["Ms"][i + 1, j] = Ms
            fa = mpf(float(albedo[j])) if albedo is not None else zero
            Is = md[-1] * fa / mp.pi + B[-1]
            mu[-1] = Is * mp.pi
            for k in range(ns):
                I, row = Is, per[k]
                if detail:
                    d["Iu"][k, nl, j] = I
                for i in range(nl - 1, -1, -1):
                    tr, s, q, _ = row[i]
                    dB = B[i + 1] - B[i]
                    I = I * tr + (B[i] * s - dB * tr + s * dB * q)
                    mu[i] += W_[k] * I
                    if detail:
                        d["Iu"][k, i, j] = I
            Mu[:, j], Md[:, j] = mu, md
            if detail:
                d["B"][:, j] = B
                d["Is"][j] = Is
                d["tau_raw"][:, j] = traw
                d["ts"][:, j] = ts
                for k in range(ns):
                    for i in range(nl):
                        tr, s, q, gg = per[k][i]
                        d["t"][k, i, j], d["s"][k, i, j], d["q"][k, i, j], d["g"][k, i, j] = tr, s, q, gg
        out = dict(tau=tau, Mup=Mu, Mdn=Md)
        if detail:
            d.update(tau=to_float(tau), Mup=to_float(Mu), Mdn=to_float(Md), nlob=nlob, W=np.array([float(x) for x in W]),
                     fa=np.zeros(nnu) if albedo is None else np.asarray(albedo, float), cth=float(cth), nl=nl, ns=ns)
            out["detail"] = d
        return out


# ---- the bound ----------------------------------------------------------------------------------------------------------------

def scan_waves(nl):
    """flux_plan (cs_api.hip): waves of the scan form"""
    return min(12, max(4, 4 * ((nl + 19) // 20)))


def scan_per(nl):
    """flux_plan: layers per wave of the scan form"""
    return -(-nl // scan_waves(nl))


def bounds(ref, arithmetic, per=None, tau_extra=0.0):
    """dict(tau, Mup, Mdn) of absolute first-order bounds, one per element of the reference's outputs (module docstring: every term).
    arithmetic: "device" or "libm"; per: layers per chunk of the scan form (None: layer by layer); tau_extra: a relative difference of
    the cross-sections a form was observed to add, carried by the tau term (0 in every form that hands sigma over bitwise)"""
    E = E_EXP[arithmetic]
    d = ref["detail"]
    nl, ns, nlob = d["nl"], d["ns"], d["nlob"]
    np_ = nl + 1
    nnu = d["tau"].shape[1]
    TINY = (30 * ns * nl + 13 * nl + 14) * 2.0 ** -1074
    rel_tau0 = (nlob + 7) * U + tau_extra
    rel_tau = np.where(d["tau_raw"] * (1 + rel_tau0) < 1e-6, 0.0, rel_tau0)                   # [nl, nnu]
    rel_q = rel_tau + (3 * U if arithmetic == "device" else 2 * U)
    B, x = d["B"], d["x"]
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        relB = U * (11 + (5 * x + E) / -np.expm1(-x))
    eB = np.where(B > 0, relB * B, 0.0) + np.where(B > 0, TINY, 0.0)
    W = d["W"][:, None]
    t, s, q, g = d["t"], d["s"], d["q"], d["g"]
    e_t = t * ((1 / q) * (rel_tau[None] + U) + E * U) + np.where(t > 0, TINY, 4 * 2.0 ** -1074)

    def step(eI, I_in, I_out, i, B1, B2, eB1, eB2):
        """all streams through layer i, entered at B1 and left at B2: the error of I_out"""
        dB = (B1 - B2)[None]
        B1, B2 = B1[None], B2[None]
        ti, si, qi, gi = t[:, i], s[:, i], q[:, i], g[:, i]
        Be = I_out - I_in * ti
        e = eI * ti + np.abs(I_in - B1 - dB * qi) * e_t[:, i] + U * si * np.abs(B2 + dB * qi)
        e += np.abs(gi) * eB1[None] + np.abs(si - gi) * eB2[None] + np.abs(gi) * U * np.abs(dB)
        e += np.abs(si * dB * qi) * rel_q[i][None]
        e += U * (np.abs(B2 * si) + np.abs(dB * ti) + 2 * np.abs(si * dB * qi) + np.abs(B2 * si - dB * ti) + np.abs(Be))
        e += U * (np.abs(I_in * ti) + np.abs(I_out)) + TINY
        return e

    def level(eI, I):
        return np.sum(W * eI, axis=0) + ns * U * np.sum(W * np.abs(I), axis=0)

    if per:
        ends = {min((w + 1) * per, nl) for w in range(-(-nl // per))}            # layer indices at which a chunk ends
    eMd, eMu = np.zeros((np_, nnu)), np.zeros((np_, nnu))
    # downward
    Id, Ms, ts = d["Id"], d["Ms"], d["ts"]
    eI = np.zeros((ns, nnu))
    eMs = (E_COS + 1) * U * Ms[0]
    eMd[0] = eMs
    A, Xin, As = np.ones((ns, nnu)), Id[:, 0], np.ones(nnu)
    for i in range(nl):
        eI = step(eI, Id[:, i], Id[:, i + 1], i, B[i], B[i + 1], eB[i], eB[i + 1])
        e_ts = ts[i] * ((d["tau"][i] / d["cth"]) * (rel_tau[i] + (E_COS + 1) * U) + E_BEAM * U) + np.where(Ms[0] > 0, TINY, 0.0)
        eMs = eMs * ts[i] + Ms[i] * e_ts + U * Ms[i + 1]
        eMd[i + 1] = level(eI, Id[:, i + 1]) + eMs + U * d["Mdn"][i + 1]
        if per:
            A, As = A * t[:, i], As * ts[i]
            if i + 1 in ends:
                eI = eI + U * (per * A * Xin + 2 * Id[:, i + 1])
                eMs = eMs + U * per * Ms[i + 1]
                A, Xin, As = np.ones((ns, nnu)), Id[:, i + 1], np.ones(nnu)
    # surface (the scan form sums the chunk-to-chunk intensities: eI, eMs carry the last boundary's roundings)
    eMd_s = level(eI, Id[:, nl]) + eMs + U * d["Mdn"][nl]
    R = d["Mdn"][nl] * d["fa"] / math.pi
    eIs = eMd_s * d["fa"] / math.pi + 3 * U * R + eB[nl] + U * d["Is"]
    eMu[nl] = math.pi * eIs + 2 * U * math.pi * d["Is"] + TINY
    # upward
    Iu = d["Iu"]
    eI = np.broadcast_to(eIs, (ns, nnu)).copy()
    A, Xin = np.ones((ns, nnu)), Iu[:, nl]
    for i in range(nl - 1, -1, -1):
        eI = step(eI, Iu[:, i + 1], Iu[:, i], i, B[i + 1], B[i], eB[i + 1], eB[i])
        eMu[i] = level(eI, Iu[:, i])
        if per:
            A = A * t[:, i]
            if i % per == 0 and i > 0:
                eI = eI + U * (per * A * Xin + 2 * Iu[:, i])
                A, Xin = np.ones((ns, nnu)), Iu[:, i]
    return dict(tau=rel_tau * d["tau"], Mup=eMu + TINY, Mdn=eMd + TINY)


def ratio(got, ref, bound):
    """worst |got - ref| / bound over the elements (the difference in 40 digits), an exact zero of the reference demanding an exact
    zero; elements whose bound is 0 must be met exactly.  A value, an error or a bound that is not finite anywhere gives inf: the
    result is never NaN"""
    got, bound = np.asarray(got, float), np.asarray(bound, float)
    if got.shape != np.shape(ref) or not (np.all(np.isfinite(got)) and np.all(np.isfinite(bound))):
        return math.inf
    with mp.workdps(40):
        err = to_float(np.abs(_mpf_arr(got) - ref))
    zero = to_float(ref) == 0.0
    if np.any(zero & (got != 0.0)) or not np.all(np.isfinite(err)):
        return math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = float(np.max(r))
    return r if math.isfinite(r) else math.inf


def ratios(got, ref, bnd):
    return {k: ratio(got[k], ref[k], bnd[k]) for k in ("tau", "Mup", "Mdn")}


def within(rr):
    """every figure of `ratios` on its own at most 1 (a NaN among them fails)"""
    return all(v <= 1.0 for v in rr.values())


# ---- the double restatement, with one planted defect ----------------------------------------------------------------------------

FAULTS = ("tau", "weights", "floor", "beam", "level1", "chunk", "albedo")


def np_fluxes(nu, P, g, muk, Tlev, sigma, S_toa, albedo, theta_s, ws, m, W, fault=None):
    """the same recurrences in plain numpy doubles, vectorised over the grid.  fault (one at a time):
      "tau"      one layer's optical depth x (1 + 1e-10): the (layer, wavenumber) whose depth is closest to 1
      "weights"  W_0 and W_1 exchanged
      "floor"    the floor at 2e-6
      "beam"     the stellar beam attenuated by exp(-tau) instead of exp(-tau / cos theta_s)
      "level1"   M- at level 1 x (1 + 1e-9)
      "chunk"    scan form: stream 0 enters the third chunk of the downward sweep without the product of the second chunk's
                 transmissivities (X + B_chunk instead of X A + B_chunk)
      "albedo"   the albedo applied to M- without the 1 / pi"""
    assert fault is None or fault in FAULTS
    nu, P, muk, Tlev, sigma = (np.asarray(a, float) for a in (nu, P, muk, Tlev, sigma))
    ws, m, W = (np.array([float(x) for x in a]) for a in (ws, m, W))
    nlob, ns, np_, nl, nnu = len(ws), len(m), len(P), len(P) - 1, len(nu)
    if fault == "weights":
        W[[0, 1]] = W[[1, 0]]
    C = 1e-4 * NA_ / g
    beta = C * (sigma / muk[:, None])
    tau = np.zeros((nl, nnu))
    for i in range(nl):
        dP = P[i + 1] - P[i]
        ti = np.zeros(nnu)
        for n in range(nlob):
            ti = ti + (dP * ws[n]) * beta[i * (nlob - 1) + n]
        tau[i] = np.maximum(ti, 2e-6 if fault == "floor" else 1e-6)
    if fault == "tau":
        i, j = np.unravel_index(np.argmin(np.abs(np.log(tau))), tau.shape)
        tau[i, j] *= 1 + 1e-10
    num = 100.0 * nu
    with np.errstate(over="ignore"):
        B = 100.0 * (2.0 * H_ * (C_ * C_) * (num * num * num))[None] / (np.exp(H_ * C_ * num[None] / (KB_ * Tlev[:, None])) - 1.0)

    def lp(B1, B2, tt, tr):
        return B2 * (1.0 - tr) - (B1 - B2) * tr + (1.0 - tr) * (B1 - B2) / tt

    c = math.cos(theta_s)
    Md, Mu = np.zeros((np_, nnu)), np.zeros((np_, nnu))
    per = scan_per(nl)
    for k in range(ns):
        I = np.zeros(nnu)
        A, X = np.ones(nnu), I
        for i in range(nl):
            tt = tau[i] * m[k]
            tr = np.exp(-tt)
            I = I * tr + lp(B[i], B[i + 1], tt, tr)
            A = A * tr
            if (i + 1) % per == 0:
                if fault == "chunk" and k == 0 and i + 1 == 2 * per:
                    I = I + (1.0 - A) * X
                A, X = np.ones(nnu), I
            Md[i + 1] += W[k] * I
    Ms = c * (np.asarray(S_toa, float) if S_toa is not None else np.zeros(nnu))
    Md[0] += Ms
    for i in range(nl):
        Ms = Ms * np.exp(-tau[i] if fault == "beam" else -tau[i] / c)
        Md[i + 1] += Ms
    if fault == "level1":
        Md[1] *= 1 + 1e-9
    fa = np.asarray(albedo, float) if albedo is not None else np.zeros(nnu)
    Is = (Md[-1] * fa if fault == "albedo" else Md[-1] * fa / math.pi) + B[-1]
    Mu[-1] = Is * math.pi
    for k in range(ns):
        I = Is
        for i in range(nl - 1, -1, -1):
            tt = tau[i] * m[k]
            tr = np.exp(-tt)
            I = I * tr + lp(B[i + 1], B[i], tt, tr)
            Mu[i] += W[k] * I
    return dict(tau=tau, Mup=Mu, Mdn=Md)


# ---- inputs -------------------------------------------------------------------------------------------------------------------

S_FULL = 10.0 ** np.linspace(-32.5, -21.4, D)      # column optical depths ~7e-8 (every layer on the floor) .. ~9e3
S_THICK = 10.0 ** np.linspace(-21.9, -20.0, D)     # every layer of the np = 9 column deeper than ~0.2: profile (b), see `case`
NU_LO, NU_HI = 14100.0, 14340.0                     # above the CO2 fixture's last line + 25 cm^-1 (asserted where the fixture is used)


def f_node(k):
    """the smooth factor in [0.5, 1.5] along the column: every Lobatto node weighs in"""
    return 1.0 + 0.5 * np.sin(0.7 * np.asarray(k, float) + 0.3)


def fmu(T, P):
    return 0.029 - 0.002 * (P / 1e5)


def profile(name, P):
    """(a) an Earth-like gradient, (b) isothermal, (c) +-40 K alternating from level to level: what Column takes as T"""
    if name == "a":
        return lambda p: 200.0 + 90.0 * (p / 1e5) ** 0.19
    if name == "b":
        return 300.0
    assert name == "c"
    return 250.0 + 40.0 * (-1.0) ** np.arange(len(P))


def _b280(v):
    return float(100.0 * 2.0 * H_ * C_ * C_ * (100.0 * v) ** 3 / math.expm1(planck_x_double(v, 280.0)))


def beam(kind):
    """fS: none, zeros, "pos" (sunlight: far brighter than the thermal emission on this grid), "thermal" (of the order of B(nu, 280 K)),
    "faint" (1e-11 of that: a beam only a per-element bound can see)"""
    return {"none": None, "zero": 0.0, "pos": lambda v: 0.4 + 0.3 * math.sin(v / 37.0),
            "thermal": lambda v: _b280(v) * (0.7 + 0.5 * math.sin(v / 37.0)),
            "faint": lambda v: 1e-11 * _b280(v) * (1.0 + 0.5 * math.sin(v / 7.0))}[kind]


def albedo_of(kind):
    return {"none": None, "zero": 0.0, "fun": lambda v: 0.05 + 0.9 * math.sin(v / 40.0) ** 2, "one": 1.0,
            "faint": lambda v: 4e-12 * (1.0 + 0.5 * math.sin(v / 5.0))}[kind]


# (fS, albedo, theta_s): every kind of each, theta_s 0 / 0.6 / 1.5
BOUNDARIES = (("none", "none", 0.6), ("zero", "zero", 0.0), ("pos", "fun", 0.6), ("pos", "one", 1.5), ("thermal", "none", 0.0),
              ("none", "fun", 0.6), ("thermal", "zero", 1.5), ("faint", "faint", 0.6))


def sigma_plane(K, nnu, sset):
    return np.asarray(sset)[np.arange(nnu) % len(sset)][None, :] * f_node(np.arange(K))[:, None]


def case(cs, prof="a", ns=4, nlob=3, np_=9, nnu=NNU_GPU, fS="pos", fa="fun", theta=0.6, sset=None, nu=None):
    """one column as the doubles an implementation is given (the library's own host functions evaluate the closures, as Column
    does).  Profile (b) takes S_THICK unless told otherwise: below a thin layer the isothermal M- is B (1 - t) with 1 - t carrying
    u / (tau m) of itself, so "accurate to a few u of itself" holds for it only where every layer is deep."""
    P = cs.pressuregrid(5.0, 1e5, np_)
    T = profile(prof, P)
    fT = cs.core.formprofile(P, T)
    Tn, mun = cs.core.lobattoevaluations(P, fT, fmu, nlob)
    Tlev = np.array([fT(p) for p in P], float)
    K = (np_ - 1) * (nlob - 1) + 1
    nu = np.linspace(NU_LO, NU_HI, nnu) if nu is None else np.asarray(nu, float)
    sset = (S_THICK if prof == "b" else S_FULL) if sset is None else sset
    ev = lambda f: None if f is None else (np.array([f(v) for v in nu], float) if callable(f) else np.full(len(nu), float(f)))
    m, W = cs.streamnodes(ns)
    return dict(nu=nu, P=P, g=G, T=T, Tn=Tn, mun=mun, muk=cs.core.nodevalues(mun, nlob), Tlev=Tlev, K=K, nlob=nlob, ns=ns,
                sigma=sigma_plane(K, len(nu), sset), fS=beam(fS), fa=albedo_of(fa), S_toa=ev(beam(fS)), albedo=ev(albedo_of(fa)),
                theta_s=theta, ws=cs.lobattonodes(nlob)[1], m=m, W=W, Pk=cs.core.nodepressures(P, nlob))


def args_of(c, **over):
    a = dict(nu=c["nu"], P=c["P"], g=c["g"], muk=c["muk"], Tlev=c["Tlev"], sigma=c["sigma"], S_toa=c["S_toa"], albedo=c["albedo"],
             theta_s=c["theta_s"], ws=c["ws"], m=c["m"], W=c["W"])
    a.update(over)
    return a


def planck_clear_of_overflow(c):
    """no Planck argument within 1e-9 of the overflow threshold, where two exponentials may fall on different sides"""
    x = planck_x_double(c["nu"][None, :], c["Tlev"][:, None])
    return bool(np.all(np.abs(x / LN_DBL_MAX - 1.0) > 1e-9))


_REF = {}


def reference(key, c, **over):
    """mp_fluxes(detail) of a case, kept under `key` for the forms that share it"""
    if key not in _REF:
        if len(_REF) >= 6:
            _REF.clear()
        _REF[key] = mp_fluxes(**args_of(c, **over), detail=True)
    return _REF[key]
