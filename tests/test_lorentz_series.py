"""The premise of the Lorentz pieces on the matrix cores (sep_step<.., LOR> in cs_kernels.h), in 40-digit arithmetic.

Far from a line the Lorentz profile is a geometric series in w = 1 / dnu^2,

    gamma / (pi (dnu^2 + gamma^2)) = (gamma / pi) sum_{n >= 0} (-gamma^2)^n w^(n+1),

which alternates: the relative truncation error after NT terms is (gamma^2 w)^NT exactly, below kSepEps from |dnu| = kSepEps^(-1/(2 NT))
gamma on.  Those are the radii sep_radii(gamma, 0) returns -- kSepR4 = 74.99 and kSepR3 = 316.3, the constants DESIGN.md quotes, times
the helper's safety factor 1 + 1e-6.  On its radius the NT-term sum is within 1e-15 of the profile and the sum of one term fewer is not,
for gamma from 1e-4 to 10 cm^-1."""
import os
import re

import mpmath as mp
import pytest

mp.mp.dps = 40

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = open(os.path.join(ROOT, "clearsky.jl_amd", "csrc", "cs_kernels.h")).read()
DESIGN = open(os.path.join(ROOT, "DESIGN.md")).read()
GAMMAS = ["1e-4", "3.7e-4", "1e-3", "0.0123", "0.07", "0.1", "0.5", "1", "2.5", "10"]
SAFE = mp.mpf(1) + mp.mpf("1e-6")      # sep_radii's `safe`


def _const(name):
    m = re.search(r"\b" + name + r"\s*=\s*([0-9.eE+-]+)\s*[,;]", KERNELS)
    assert m, name
    return m.group(1)


def _radius(nt):
    """the radius per unit gamma of the NT-term series, restated from kSepEps: eps^(-1/(2 NT)) rounded up to four digits"""
    eps = mp.mpf(_const("kSepEps"))
    r = eps ** (mp.mpf(-1) / (2 * nt))
    digits = 4 - (int(mp.floor(mp.log10(r))) + 1)
    return mp.ceil(r * 10 ** digits) / 10 ** digits


def _partial(gamma, dnu, nt):
    w = 1 / dnu ** 2
    return gamma / mp.pi * sum((-gamma ** 2) ** n * w ** (n + 1) for n in range(nt))


def test_radii_are_the_quoted_constants():
    assert mp.mpf(_const("kSepEps")) == mp.mpf("1e-15")
    for nt, quoted in ((4, "74.99"), (3, "316.3")):
        assert _radius(nt) == mp.mpf(_const(f"kSepR{nt}")) == mp.mpf(quoted), nt
        assert quoted in DESIGN
    # at alpha = 0 the helper's radius is kSepR_n gamma (1 + 1e-6): sqrt(g2 + kSepA_n a2) with a2 = 0
    assert re.search(r"kSepR4 \* sqrt\(g2 \+ kSepA4 \* a2\) \* safe", KERNELS) and re.search(r"kSepR3 \* sqrt\(g2 \+ kSepA3 \* a2\) \* safe", KERNELS)


@pytest.mark.parametrize("nt", [4, 3])
@pytest.mark.parametrize("gamma", GAMMAS)
def test_series_on_its_radius(nt, gamma):
    g = mp.mpf(gamma)
    eps = mp.mpf(_const("kSepEps"))
    for sign in (1, -1):
        dnu = sign * _radius(nt) * g * SAFE
        exact = g / (mp.pi * (dnu ** 2 + g ** 2))
        err = abs(_partial(g, dnu, nt) / exact - 1)
        short = abs(_partial(g, dnu, nt - 1) / exact - 1)
        assert err <= eps, (nt, gamma, err)
        assert short > eps, (nt, gamma, short)
        # the series is geometric: the error is (gamma^2 w)^NT itself (a 1e-15 difference of 40-digit numbers keeps 25 digits)
        assert abs(err / (g ** 2 / dnu ** 2) ** nt - 1) < mp.mpf(10) ** -20
