"""The radii of the matrix-core series (sep_radii in cs_kernels.h) against the boundary samples of tools/voigt_series.py.

tests/golden/series_radii.json holds, for the 3-, 4- and 8-term series, lines sitting exactly on their own radius (y from 1e-3 to 100) with
40-digit values of sqrt(pi) K(x,y)/y.  The truncated series evaluated in float64 in the device's order must be within 2e-15 of them (1e-15
of truncation, the rest rounding), and the constants compiled into the library must be the ones the tool derives from kSepEps."""
import json
import os
import re
import sys
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import voigt_series as VS  # noqa: E402

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "series_radii.json")))
KERNELS = open(os.path.join(ROOT, "clearsky.jl_amd", "csrc", "cs_kernels.h")).read()


def _const(name):
    m = re.search(r"\b" + name + r"\s*=\s*([0-9.eE+-]+)\s*[,;]", KERNELS)
    assert m, name
    return float(m.group(1))


@pytest.mark.parametrize("n", [3, 4, 8])
def test_series_on_the_boundary_float64(n):
    rows = [s for s in GOLD["samples"] if s["n"] == n]
    assert len(rows) >= 40
    ys = sorted(s["y2"] for s in rows)
    assert ys[0] <= 1.1e-6 and ys[-1] >= 0.99e4                   # y from 1e-3 to 100
    worst = 0.0
    for s in rows:
        ref = Fraction(s["ref"])
        got = Fraction(VS.series_f64(n, s["y2"], s["dd"], s["dnu"]))
        worst = max(worst, float(abs(got / ref - 1)))
    assert worst <= 2e-15, worst


@pytest.mark.parametrize("n", [3, 4, 8])
def test_samples_sit_on_the_radius(n):
    const = VS.constants(GOLD["eps"])
    for s in (s for s in GOLD["samples"] if s["n"] == n):
        alpha = VS.SQLN2 / s["dd"]
        gamma = s["y2"] ** 0.5 / s["dd"]
        assert VS.radius(n, gamma, alpha, const) == pytest.approx(s["dnu"], rel=1e-12)


def test_device_constants_match_the_tool():
    eps = _const("kSepEps")
    assert eps == GOLD["eps"] <= 1e-15                             # never looser than the vector-unit far bodies
    const = VS.constants(eps)
    for n in (3, 4, 8):
        assert _const(f"kSepR{n}") == const[n][0] == GOLD["radii"][str(n)]["kSep"], n
        assert _const(f"kSepA{n}") == const[n][1] == GOLD["radii"][str(n)]["alpha_factor"], n
        assert const[n][0] >= eps ** (-0.5 / n) and const[n][1] >= VS.A_N[n] / 0.6931471805599453
    # every zone routine takes its radii from the one helper: no radius is written out anywhere else
    assert len(re.findall(r"kSepR[348]\s*\*", KERNELS)) == 3
    assert not re.search(r"\b(133\.6|682\.0|11\.55)\b", KERNELS)
    assert KERNELS.count("sep_radii(gb, amax)") == 2               # izone_compute, and state_radii for both piece tables
