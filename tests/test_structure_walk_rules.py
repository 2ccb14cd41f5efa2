"""The conditions that keep the walks of tests/test_gpu_structure_walk.py from being vacuous, from their step tables alone: a context
walked through structures that only ever grow, or that never change the padding of the node sums, would find no residue.  No GPU needed."""
import os
import re

import pytest

import test_gpu_structure_walk as S
import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALKS = {"voigt-forms": S.VOIGT_FORMS, "flux-forms": S.FLUX_FORMS, "shape-codes": S.SHAPE_CODES, "absorber-kinds": S.ABSORBER_KINDS,
         "precision": S.PRECISION}
RESIDENT = [S.I_COLUMN, S.I_PH_COLUMN]


def _kpad():
    """cheb_kpad of clearsky.jl_amd/csrc: K rounded up to CS_KPAD states"""
    with open(os.path.join(ROOT, "clearsky.jl_amd", "csrc", "cs_kernels.h"), encoding="utf-8") as f:
        n = int(re.search(r"#define CS_KPAD (\d+)", f.read()).group(1))
    with open(os.path.join(ROOT, "clearsky.jl_amd", "csrc", "cs_api.hip"), encoding="utf-8") as f:
        assert "int cheb_kpad(int K) { return (K + CS_KPAD - 1) / CS_KPAD * CS_KPAD; }" in f.read()
    return n, (lambda K: (K + n - 1) // n * n)


@pytest.mark.parametrize("name", list(WALKS))
def test_sizes_fall_and_rise(name):
    """K nnu (records' states, sigma, the near-line plane), nl nnu (tau) and np nnu (M+, M-) each fall at least once and rise at least once
    between consecutive steps: every plane is at some step smaller than what the context already holds"""
    steps = WALKS[name]
    for what, size in (("K nnu", lambda s: s.K * s.nnu), ("nl nnu", lambda s: s.nl * s.nnu), ("np nnu", lambda s: s.npl * s.nnu)):
        v = [size(s) for s in steps]
        assert any(b < a for a, b in zip(v, v[1:])), (name, what, v)
        assert any(b > a for a, b in zip(v, v[1:])), (name, what, v)


@pytest.mark.parametrize("name", ["voigt-forms", "flux-forms"])
def test_padding_states_change(name):
    """cheb_kpad(K), or the number of padding states behind K, differs between some pair of neighbours"""
    n, kpad = _kpad()
    assert n == 16
    steps = WALKS[name]
    assert any(kpad(a.K) != kpad(b.K) or a.K % n != b.K % n for a, b in zip(steps, steps[1:])), [s.K for s in steps]
    if name == "voigt-forms":      # (both: a larger padded block before a smaller one, and the other way)
        pads = [kpad(s.K) for s in steps]
        assert any(b < a for a, b in zip(pads, pads[1:])) and any(b > a for a, b in zip(pads, pads[1:])), pads


@pytest.mark.parametrize("name", list(WALKS))
def test_returns_to_the_first_structure(name):
    steps = WALKS[name]
    assert steps[-1] is steps[0] and len(steps) > 2
    assert all(a is not b for a, b in zip(steps, steps[1:]))      # (no step repeats its neighbour)
    labels = {}
    for s in steps:                                                # (a label names one structure: the walk keys its visits by it)
        assert labels.setdefault(s.label, s) is s, s.label


def test_every_settings_record_is_complete():
    for s in [s for steps in WALKS.values() for s in steps] + RESIDENT:
        assert tuple(s.settings) == S.SETTINGS_KEYS, s.label
        assert tuple(sorted(s.settings["tuning"])) == S.TUNE_KEYS, s.label
    d = S.settings()      # the defaults are cs_create's (clearsky.jl_amd/csrc/cs_api.hip: cs_ctx and Settings)
    assert (d["precision"], d["far_s"], d["set_interp"], d["set_interp_plan"], d["set_matrix_cores"], d["set_merge"]) == \
        ("fp64", 1e6, True, (-1, 128, 2048), 1, True)
    assert d["tuning"] == {4: 0, 7: 1, 15: 0}
    with open(os.path.join(ROOT, "clearsky.jl_amd", "csrc", "cs_api.hip"), encoding="utf-8") as f:
        src = f.read()
    for text in ("int mixed = 0;", "double far_s = 1e6;", "int interp = 1;", "int itp_first = -1, itp_min = 128, itp_max = 2048;", "int merge = 1;",
                 "int matrix_nodes = 1;", "bool matrix_core = true;", "bool graph = false;", "int near_stream = 1;", "int flux_form = 0;"):
        assert text in src, text


def test_interleaved_calls_outgrow_the_column():
    """the conditions under which a workspace shared between the resident column and the other entry points would be reallocated: the
    shape call needs K L records beyond the column's K maxL, the batch B K states beyond its K"""
    c = S.I_COLUMN
    maxL = len(W.lines("fixture", "CO2").nu) + len(W.lines("fixture", "H2O").nu)       # (one merged Voigt group)
    L = len(W.lines(*S.I_SHAPE_TABLE).nu)
    assert L > maxL and S.I_SHAPE_STATES > c.K
    assert S.I_SHAPE_STATES * L > c.K * maxL
    assert S.I_BATCH * c.K > c.K and S.I_BATCH == 3
    assert S.I_PH_STATES > S.I_PH_COLUMN.K
