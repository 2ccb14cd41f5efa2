"""The chunk rules of tests/test_gpu_state_chunks.py (RULES) against clearsky.jl_amd/csrc/cs_api.hip: the per-state bytes and the kc
expressions of gas_states -- the state-chunked driver behind cs_shape_batch / cs_shape_points (shape_impl), which have it own the chunk's
sigma, and cs_bake, which has it write the table's plane in place -- and of cs_column_batch, the pedestal workspace and the record sizes
they count.  If one of them changes, the GPU tests may no longer cross a chunk boundary; this fails first.  No GPU needed."""
import os
import re

import numpy as np

import test_gpu_state_chunks as SC
import voigt_lbl_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clearsky.jl_amd", "csrc")

# the two sides of the driver's per-state bytes: Z is the caller's device plane (NULL: the driver owns the chunk's sigma)
OWNED = "(size_t)nnu * (sizeof(double) + kNearPointBytes)"   # rule "shape"
IN_PLACE = "(size_t)nnu * kNearPointBytes"                   # rule "bake"
# function -> (rules, per-state bytes, kc) as written in the source, whitespace collapsed
SOURCE = {
    "static int gas_states(": (("shape", "bake"),
        "const size_t per_state = (size_t)G.L * (sizeof(LineHot) + sizeof(LineCold)) + "
        "(Z ? " + IN_PLACE + " : " + OWNED + ") + (ped ? ped_bytes(1, G.L) : 0);",
        "const int kc = (int)std::max<size_t>(1, std::min<size_t>({(size_t)K, ((size_t)4 << 30) / per_state, (size_t)65535}));"),
    "int cs_column_batch(": (("column",),
        "const size_t per_state = maxL * (sizeof(LineHot) + sizeof(LineCold) + (ctx->mixed ? sizeof(LineF32) : 0)) + "
        "(size_t)c.nnu * kNearPointBytes + (any_ped ? ped_bytes(1, (int64_t)maxL) : 0) + (vvh2 ? (size_t)c.nnu * sizeof(double) : 0);",
        "const int kc = (int)std::max<size_t>(1, std::min<size_t>({(size_t)BK, ((size_t)8 << 30) / std::max<size_t>(per_state, 1), "
        "(size_t)65535}));"),
}


def _norm(s):
    return re.sub(r"\s+", " ", s)


def _read(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def _body(src, head):
    """the text of the function whose definition (not a declaration) starts with head, up to the next top-level closing brace"""
    i = src.index(head)
    while src.index(";", i) < src.index("{", i):
        i = src.index(head, i + 1)
    j = src.index("\n}\n", i)
    return _norm(src[i:j])


def test_kc_expressions_match_the_rule_table():
    src = _read("cs_api.hip")
    for head, (rule, per_state, kc) in SOURCE.items():
        body = _body(src, head)
        assert _norm(per_state) in body, (rule, "per-state bytes")
        assert _norm(kc) in body, (rule, "kc")
        assert re.search(r"for \(int(64_t)? k0 = 0; k0 < (K|M|BK); k0 \+= kc\)", body), (rule, "chunk loop")
    assert {r for rules, _, _ in SOURCE.values() for r in rules} == set(SC.RULES)
    # which side of the driver's conditional term an entry point takes: Z is what out.plane hands out, and only cs_bake sets one
    drv = _body(src, "static int gas_states(")
    assert "double *Z = nullptr;" in drv and "if (out.plane && (rc = out.plane(Z))) return rc;" in drv
    assert drv.count("Z = ") == 1 and "dsig.reserve((size_t)kc * nnu * sizeof(double))" in drv
    shape = _body(src, "static int shape_impl(")
    assert "out.host = sigma; out.ld = ld_state;" in shape and "plane =" not in shape and "gas_states(ctx, ctx->gas[slot]," in shape
    for head in ("int cs_shape_batch(", "int cs_shape_points("):
        assert "return shape_impl(ctx, slot, shape," in _body(src, head), head
    bake = _body(src, "int cs_bake(")
    assert "out.plane = [&](double *&Z) {" in bake and "Z = tb.Z.as<double>();" in bake and "out.host" not in bake
    assert "gas_states(ctx, ctx->gas[gas_slot]," in bake
    # ... and the two sides are the rules' own terms, on top of the same record and pedestal bytes
    L, n = SC.NLINES, 400
    for ped in (False, True):
        common = L * (SC.HOT + SC.COLD) + (SC.ped_bytes(1, L) if ped else 0)
        assert SC.RULES["shape"][1](L, n, ped=ped) == common + n * (SC.DBL + SC.INT2)
        assert SC.RULES["bake"][1](L, n, ped=ped) == common + n * SC.INT2
    budgets = {r: b for r, (b, _) in SC.RULES.items()}
    assert budgets == {"shape": 4 << 30, "bake": 4 << 30, "column": 8 << 30}
    assert SC.GRID_Y == 65535
    # the column's second code-5/6 plane: the groups are ordered codes 5/6 first, so group 1 is one when there are two
    assert "const bool vvh2 = c.gas.size() > 1 && c.gas[1].vvh;" in src


def test_sizes_the_rules_count():
    src = _read("cs_api.hip")
    k = _norm(_read("cs_kernels.h"))
    assert "static size_t ped_bytes(int64_t kn, int64_t L) { return (size_t)kn * ((size_t)3 * L + (L + CS_PED_B - 1) / CS_PED_B) * " \
           "sizeof(double); }" in _norm(src)
    assert re.search(r"#define CS_PED_B (\d+)", k).group(1) == str(SC.PED_B)
    assert "struct __attribute__((aligned(32))) LineHot { double nul, p1, p2, p3; };" in k and SC.HOT == 32
    # the two 32-bit range words of a (state, point) in the near-line hand-off (NearHandoff): the INT2 of the rules
    assert "constexpr size_t kNearPointBytes = 2 * sizeof(unsigned);" in k and SC.INT2 == 2 * 4
    assert "struct __attribute__((aligned(16))) LineCold { double y, A; };" in k and SC.COLD == 16
    assert "struct __attribute__((aligned(16))) LineF32 { float d, y2, ay, c2; };" in k and SC.F32 == 16
    assert SC.ped_bytes(1, 100) == (300 + 2) * 8


def test_rule_arithmetic():
    """the table's own arithmetic on the tests' inputs: 400 000 lines on a 400-point grid"""
    L, n = SC.NLINES, 400
    assert SC.chunk_size("shape", 10 ** 6, L, n) == (4 << 30) // (L * 48 + n * 16)
    assert SC.chunk_size("bake", 10 ** 6, L, n, ped=True) == (4 << 30) // (L * 48 + n * 8 + (3 * L + -(-L // 64)) * 8)
    assert SC.chunk_size("column", 10 ** 6, L, n, mixed=True, vvh2=True) == (8 << 30) // (L * 64 + n * 8 + n * 8)
    assert SC.chunk_size("shape", 70000, 20, 64) == 65535 and SC.chunk_size("shape", 100, 20, 64) == 100
    for rule, kw in (("shape", {}), ("shape", {"ped": True}), ("bake", {}), ("column", {"vvh2": True, "ped": True}), ("column", {"mixed": True})):
        for step in (1, 17, 31):
            N = SC.states_for(rule, L, n, step=step, **kw)
            assert N % step == 0
            kc, b = SC.boundaries(rule, N, L, n, **kw)
            assert len(b) == 2 and b == [kc, 2 * kc]


def test_shifted_cases_cross_chunks_and_see_their_shifts():
    """the shifted cases of test_gpu_state_chunks.py, without a GPU: every one makes three chunks with a ragged last one (boundaries():
    with 10 % fewer bytes per state too); the largest pressure, so the largest shift ds, belongs to no state of the first chunk; the
    compared rows are exact in fp64 (the premise of the 1e-11 bar); and among them membership by shifted centre differs from membership
    by table position for the direct and the mirror terms, and the strict pre-filter keeps a line in one row that it drops in another"""
    t = SC.shifted_lines()
    nul, da, nu = t["nu"], t["delta_a"], SC.GRID_DY
    L = len(nul)
    assert 300_000 < L <= SC.NLINES and np.all(nul * 64 == np.round(nul * 64)) and np.all(da * 32 == np.round(da * 32))
    assert np.max(np.abs(da)) == 0.1875 and np.mean(np.diff(nul + da * 2.0) < 0) > 0.01      # neighbours swap their order at 2 atm
    for code, cut in SC.SHIFT_CASES:
        ped = code == 7
        c = SC.shift_case(code, cut)
        assert c.b0 == [c.kc, 2 * c.kc] and c.kc == SC.chunk_size("shape", c.n, L, len(nu), ped=ped)
        assert np.max(c.P[:c.kc]) == 0.5 * SC.KATM and np.max(c.P) == 2.0 * SC.KATM and all(c.P[k0] == 2.0 * SC.KATM for k0 in c.b0)
        assert 0.1875 * 2.0 == 0.375 and (cut == 0.25) == (cut < 0.375)
        assert {0, c.n - 1, c.kc - 1, c.kc, 2 * c.kc - 1, 2 * c.kc} <= set(c.rows) and sum(c.P[k] >= 0.25 * SC.KATM for k in c.rows) >= 4
        a, b = np.searchsorted(nul, [max(0.0, nu[0] - cut - 1.0), nu[-1] + cut + 1.0])       # (_reach)
        V.dyadic_premise(nul[a:b], nu, da[a:b], np.unique(c.P[c.rows]))
        direct = mirror = any_mirror = False
        keep = []
        for k in c.rows:
            d, m, d0, m0 = V.membership(nul[a:b], da[a:b], nu, c.P[k], cut)
            direct, mirror, any_mirror = direct or bool(np.any(d != d0)), mirror or bool(np.any(m != m0)), any_mirror or bool(np.any(m | m0))
            cen = nul[a:b] + da[a:b] * c.P[k] / SC.KATM
            keep.append((cen > nu[0] - cut) & (cen < nu[-1] + cut))
        keep = np.array(keep)
        assert direct, (code, cut)
        assert np.any(keep.any(axis=0) & ~keep.all(axis=0)), (code, cut)
        if code == 7:   # (the flagged codes 0-2 have no mirror term; at cut 0.25 < nu_1 no mirror line exists on this grid)
            assert mirror == any_mirror == (cut > nu[0]), (code, cut)
    for code in SC.BAKE_SHIFT_CASES:
        nP, n, kc, b0 = SC.bake_sizes(code)
        assert n == SC.NT_BAKE * nP and b0 == [kc, 2 * kc] and kc == SC.chunk_size("bake", n, L, len(nu), ped=code == 7)
    for code, kw in [(c_, {}) for c_, _ in SC.COLUMN_SHIFT_CASES] + [(7, dict(vvh2=True))]:
        B, kc, b0 = SC.column_sizes(code, **kw)
        assert b0 == [kc, 2 * kc] and any(k0 % SC.NP_COL for k0 in b0)
        assert kc == SC.chunk_size("column", B * SC.NP_COL, L, len(nu), ped=code == 7, **kw)
