#!/usr/bin/env python3
"""Cost of the radiation-term flag of CIA objects (CS_CIA_RADIATION) on one MI355X: tools/continuum_cost.py [--steps 20] [--bench FILE ...] [--out profiles/continuum_cost.json]

Cases (the C5 column, BASELINE configs[4]: H2O + CO2 + CH4 + O3 line by line and the CO2-CO2 and CO2-CH4 CIA files, 5e5 nu x 100
layers, Discretized(5, 2), band fluxes only):
  cia            both CIA objects as they are (the kernels every column without a flagged object runs)
  cia_radiation  both flagged: R(nu, T_k) = nu tanh(c2 nu / 2T_k) multiplies their band sums -- one tanh per (point, state, object) where
                 a band reaches the point (as a measurement of cost: a CIA file is no continuum coefficient)
The median of `steps` steps after 3 warm-up steps (host wall clock around run + sync), the cases' steps interleaved.  --bench NAME=FILE
adds the headline (ms_per_step) of bench.py result lines saved in FILE under NAME, with the spread of the runs in it."""
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


def column(cfg, radiation):
    ctx = cs.Context(0)
    members = [cs.CIATables(a.filename, extrapolate=a.extrapolate, singles=a.singles, radiation=radiation) if isinstance(a, cs.CIATables) else a
               for a in cfg["absorbers"]]
    col = cs.Column(cfg["P"], cfg["g"], cfg["T"], cfg["mu"], cfg["fS"], cfg["fa"], *members, core=cfg["core"], ctx=ctx, want_tau=False, want_M=False)
    return ctx, col


def timed(cols, steps, warmup=3):
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
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), flux_form=cols[k].info()["flux_form"],
                    launches=cols[k].info()["launches"], Fup_toa=float(cols[k].fetch()[0][0])) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--bench", action="append", default=[], metavar="NAME=FILE")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "continuum_cost.json"))
    a = ap.parse_args()
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out.update({"what": __doc__.splitlines()[0], "build_id": cs.lib().cs_build_id().decode()})
    for spec in a.bench:
        name, path = spec.split("=", 1)
        runs = [json.loads(ln) for ln in open(path) if ln.lstrip().startswith("{")]
        ms = [r["ms_per_step"] for r in runs]
        out[f"bench_{name}"] = dict(ms_per_step=ms, median_ms=float(np.median(ms)), spread_ms=float(np.max(ms) - np.min(ms)),
                                    build_id=runs[0].get("kernel_source_sha16"))
    if a.steps > 0:
        cfg = W.config("C5")
        made = {"cia": column(cfg, False), "cia_radiation": column(cfg, True)}
        res = timed({k: m[1] for k, m in made.items()}, a.steps)
        for k, r in res.items():
            out[f"c5_{k}"] = r
        out["c5_ratio"] = res["cia_radiation"]["median_ms"] / res["cia"]["median_ms"]
        for ctx, _ in made.values():
            ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
