#!/usr/bin/env python3
"""Cost of shape code 7 (LBLRTM's line calculation at pressure-shifted centres) against code 6 and the flagged code 0 on one MI355X: tools/voigt_lbl_cost.py [--steps 30] [--out profiles/voigt_lbl_cost.json]

Cases (the C3 column: 1e5 nu x 60 layers, synthetic H2O + CO2 tables, Discretized(5, 2), band fluxes only).  The H2O table goes through a
.par file (the library takes the shifts from the file alone), its shifts drawn from the multiples of 2^-5 in [-0.1875, 0.125] cm^-1/atm
-- the range of the golden H2O file:
  voigtCKDVVH    H2O as code 6, CO2 as code 0: two groups, H2O's on the matrix cores
  voigt_pshift   H2O as code 0 | CS_SHAPE_PSHIFT, CO2 as code 0: two groups, H2O's on the vector path (no matrix-core pieces)
  voigtLBL       H2O as code 7, CO2 as code 0: two groups; the flagged group's line sum, then code 6's finish pass by shifted centres
for the whole grid and its 4th 1/8 nu-shard, the median of `steps` steps after 5 warm-up steps (host wall clock around run + sync), the
cases' steps interleaved so that clock drift falls on all of them alike."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import clearsky_jl_amd as cs   # noqa: E402
import workloads as W          # noqa: E402

CASES = {"voigtCKDVVH": ("voigtCKDVVH", False), "voigt_pshift": ("voigt", True), "voigtLBL": ("voigtLBL", False)}


def _fx(x, w, dec):
    r = f"{x:.{dec}f}"
    if len(r) > w:
        r = r.replace("0.", ".", 1)
    assert len(r) <= w, (x, w)
    return r.rjust(w)


def par_copy(sl, path, seed=5):
    """sl's lines as a HITRAN 160-column file (first isotopologue) with seeded shifts, read back"""
    rng = np.random.default_rng(seed)
    da = rng.integers(-6, 5, len(sl.nu)) / 32.0
    with open(path, "w") as f:
        for j in range(len(sl.nu)):
            r = (f"{int(sl.M):2d}1{sl.nu[j]:12.6f}{sl.S[j]:10.3E}{1.0:10.3E}{_fx(sl.gamma_a[j], 5, 4)}{_fx(sl.gamma_s[j], 5, 3)}"
                 f"{sl.Epp[j]:10.4f}{_fx(sl.na[j], 4, 2)}{_fx(da[j], 8, 5)}")
            assert len(r) == 67, r
            f.write(r + " " * 93 + "\n")
    return cs.SpectralLines(path)


def column(cfg, h2o, shape, flag, nu_range=None):
    ctx = cs.Context(0)
    gases = [cs.DirectGas(h2o, cfg["absorbers"][0].fC, cfg["nu"], shape=shape, pressure_shift=flag),
             cs.DirectGas(cfg["absorbers"][1].sl, cfg["absorbers"][1].fC, cfg["nu"])]
    col = cs.Column(cfg["P"], cfg["g"], cfg["T"], cfg["mu"], cfg["fS"], cfg["fa"], *gases, core=cfg["core"], ctx=ctx,
                    want_tau=False, want_M=False, nu_range=nu_range)
    return ctx, col


def timed(cols, steps, warmup=5):
    for _ in range(warmup):
        for c in cols.values():
            c.run()
            c.sync()
    t = {k: [] for k in cols}
    for _ in range(steps):
        for k, c in cols.items():
            t0 = time.perf_counter()
            c.run()
            c.sync()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), groups=cols[k].info()["groups"],
                    launches=cols[k].info()["launches"], flux_form=cols[k].info()["flux_form"]) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voigt_lbl_cost.json"))
    a = ap.parse_args()
    cfg = W.config("C3")
    out = {"what": __doc__.splitlines()[0], "cases": {k: f"H2O as {v[0]}{' | CS_SHAPE_PSHIFT' if v[1] else ''}, CO2 as voigt" for k, v in CASES.items()},
           "build_id": cs.lib().cs_build_id().decode()}
    with tempfile.TemporaryDirectory() as tmp:
        h2o = par_copy(cfg["absorbers"][0].sl, os.path.join(tmp, "h2o.par"))
        n = len(cfg["nu"])
        shard = (3 * n // 8, 4 * n // 8)
        for name, rng in (("full", None), ("shard_1_of_8", shard)):
            made = {k: column(cfg, h2o, *v, nu_range=rng) for k, v in CASES.items()}
            res = timed({k: m[1] for k, m in made.items()}, a.steps)
            for k, r in res.items():
                out[f"{name}_{k}"] = r
            out[f"{name}_ratio_vs_code6"] = res["voigtLBL"]["median_ms"] / res["voigtCKDVVH"]["median_ms"]
            out[f"{name}_ratio_vs_flagged_code0"] = res["voigtLBL"]["median_ms"] / res["voigt_pshift"]["median_ms"]
            for ctx, _ in made.values():
                ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if "ratio" in k}))


if __name__ == "__main__":
    main()
