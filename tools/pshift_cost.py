#!/usr/bin/env python3
"""Cost of the pressure-shift flag (CS_SHAPE_PSHIFT) on one MI355X: tools/pshift_cost.py --part {full,shard,bake} [--steps 30] [--out profiles/pressure_shift_cost.json]

Cases (the C3 column: 1e5 nu x 60 layers, synthetic H2O + CO2 tables, Discretized(5, 2), band fluxes only):
  voigt          H2O and CO2 as code 0, merged into one launch group (the library default)
  voigt_pshift   H2O as code 0 | CS_SHAPE_PSHIFT, CO2 as code 0: two groups (a flagged gas merges only with flagged gases)
The library takes the shifts from a .par file, so the synthetic H2O table is written as one first, its delta_a drawn from the golden
H2O file's (both cases run on the table read back).  Parts: `full` the whole grid, `shard` its 4th 1/8 nu-shard -- the median of `steps`
steps after 5 warm-up steps (host wall clock around run + sync), the cases' steps interleaved -- and `bake` a 12 x 24 bake of the H2O
table on the C3 grid with and without the flag.  Each part adds its entries to the output file."""
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


def _fx(x, w, dec):
    r = f"{x:.{dec}f}"
    if len(r) > w:
        r = r.replace("0.", ".", 1)
    return r.rjust(w)


def shifted_h2o(sl, path):
    """sl written as a HITRAN .par file with delta_a resampled from the golden H2O file, and read back"""
    da = np.random.default_rng(1).choice(cs.SpectralLines(os.path.join(ROOT, "tests", "golden", "hitran", "H2O.par")).delta_a, len(sl.nu))
    with open(path, "w") as f:
        for j in range(len(sl.nu)):
            f.write(f"{sl.M:2d}{int(sl.I[j]) % 10:1d}{sl.nu[j]:12.6f}{sl.S[j]:10.3E}{1.0:10.3E}{_fx(sl.gamma_a[j], 5, 4)}{_fx(sl.gamma_s[j], 5, 3)}"
                    f"{sl.Epp[j]:10.4f}{_fx(sl.na[j], 4, 2)}{_fx(da[j], 8, 5)}" + " " * 93 + "\n")
    return cs.SpectralLines(path)


def column(cfg, h2o, flag, nu_range=None):
    ctx = cs.Context(0)
    gases = [cs.DirectGas(h2o, cfg["absorbers"][0].fC, cfg["nu"], pressure_shift=flag),
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
                    launches=cols[k].info()["launches"], flux_form=cols[k].info()["flux_form"],
                    line_kernel=cols[k].info()["line_kernel"]) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("full", "shard", "bake"), required=True)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pressure_shift_cost.json"))
    a = ap.parse_args()
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out.update({"what": __doc__.splitlines()[0], "build_id": cs.lib().cs_build_id().decode(),
                "cases": {"voigt": "H2O and CO2 as code 0 (merged)", "voigt_pshift": "H2O as code 0 | CS_SHAPE_PSHIFT, CO2 as code 0"}})
    cfg = W.config("C3")
    with tempfile.TemporaryDirectory() as d:
        h2o = shifted_h2o(cfg["absorbers"][0].sl, os.path.join(d, "h2o_synthetic.par"))
        n = len(cfg["nu"])
        if a.part in ("full", "shard"):
            rng = None if a.part == "full" else (3 * n // 8, 4 * n // 8)
            name = "full" if a.part == "full" else "shard_1_of_8"
            made = {"voigt": column(cfg, h2o, False, rng), "voigt_pshift": column(cfg, h2o, True, rng)}
            res = timed({k: m[1] for k, m in made.items()}, a.steps)
            for k, r in res.items():
                out[f"{name}_{k}"] = r
            out[f"{name}_ratio"] = res["voigt_pshift"]["median_ms"] / res["voigt"]["median_ms"]
            for ctx, _ in made.values():
                ctx.close()
        else:
            ctx = cs.Context(0)
            Om = cs.AtmosphericDomain((150.0, 350.0), 12, (10.0, 1e5), 24)
            for flag in (False, True):
                cs.Gas(h2o, 0.01, cfg["nu"], Om, ctx=ctx, pressure_shift=flag)   # (first call: allocations)
                t0 = time.perf_counter()
                cs.Gas(h2o, 0.01, cfg["nu"], Om, ctx=ctx, pressure_shift=flag)
                out[f"bake_12x24_{'pshift' if flag else 'voigt'}_s"] = time.perf_counter() - t0
            ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k.endswith("ratio") or k.startswith("bake") or k.endswith("median_ms")}))


if __name__ == "__main__":
    main()
