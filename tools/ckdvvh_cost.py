#!/usr/bin/env python3
"""Cost of shape code 6 (pedestal-removed Van Vleck-Huber Voigt) against codes 5 and 0 on one MI355X: tools/ckdvvh_cost.py [--steps 30] [--out profiles/voigt_ckdvvh_cost.json]

Cases (the C3 column: 1e5 nu x 60 layers, synthetic H2O + CO2 tables, Discretized(5, 2), band fluxes only):
  voigt          H2O and CO2 as code 0, merged into one launch group (the library default)
  voigt_nomerge  the same with merging off: two launch groups
  voigtVVH       H2O as code 5, CO2 as code 0: two groups (code 5 is never merged with code 0)
  voigtCKDVVH    H2O as code 6, CO2 as code 0: two groups (code 6 is never merged with code 0)
  voigtCKD       H2O as code 4, CO2 as code 0: two groups (code 4 is never merged with code 0); the case of profiles/voigt_ckd_cost.json
for the whole grid and its 4th 1/8 nu-shard, the median of `steps` steps after 5 warm-up steps (host wall clock around run + sync), the
cases' steps interleaved so that clock drift falls on all of them alike; and a 12 x 24 bake of the H2O table on the C3 grid as codes 0, 5 and 6."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import clearsky_jl_amd as cs   # noqa: E402
import workloads as W          # noqa: E402

CASES = {"voigt": ("voigt", True), "voigt_nomerge": ("voigt", False), "voigtVVH": ("voigtVVH", True),
         "voigtCKDVVH": ("voigtCKDVVH", True), "voigtCKD": ("voigtCKD", True)}


def column(cfg, shape, merge, nu_range=None):
    ctx = cs.Context(0)
    ctx.set_merge(merge)
    gases = [cs.DirectGas(g.sl, g.fC, cfg["nu"], shape=shape if i == 0 else "voigt") for i, g in enumerate(cfg["absorbers"])]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voigt_ckdvvh_cost.json"))
    a = ap.parse_args()
    cfg = W.config("C3")
    out = {"what": __doc__.splitlines()[0], "cases": {k: f"H2O as {v[0]}, merge {'on' if v[1] else 'off'}" for k, v in CASES.items()},
           "build_id": cs.lib().cs_build_id().decode()}
    n = len(cfg["nu"])
    shard = (3 * n // 8, 4 * n // 8)
    for name, rng in (("full", None), ("shard_1_of_8", shard)):
        made = {k: column(cfg, *v, nu_range=rng) for k, v in CASES.items()}
        res = timed({k: m[1] for k, m in made.items()}, a.steps)
        for k, r in res.items():
            out[f"{name}_{k}"] = r
        out[f"{name}_overhead_vs_code5"] = res["voigtCKDVVH"]["median_ms"] / res["voigtVVH"]["median_ms"] - 1.0
        out[f"{name}_overhead"] = res["voigtCKDVVH"]["median_ms"] / res["voigt"]["median_ms"] - 1.0
        out[f"{name}_overhead_vs_unmerged"] = res["voigtCKDVVH"]["median_ms"] / res["voigt_nomerge"]["median_ms"] - 1.0
        for ctx, _ in made.values():
            ctx.close()
    ctx = cs.Context(0)
    Om = cs.AtmosphericDomain((150.0, 350.0), 12, (10.0, 1e5), 24)
    h2o = cfg["absorbers"][0].sl
    for shape in ("voigt", "voigtVVH", "voigtCKDVVH"):
        cs.Gas(h2o, 0.01, cfg["nu"], Om, shape=shape, ctx=ctx)   # (first call: allocations)
        t0 = time.perf_counter()
        cs.Gas(h2o, 0.01, cfg["nu"], Om, shape=shape, ctx=ctx)
        out[f"bake_12x24_{shape}_s"] = time.perf_counter() - t0
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if "overhead" in k or k.startswith("bake")}))


if __name__ == "__main__":
    main()
