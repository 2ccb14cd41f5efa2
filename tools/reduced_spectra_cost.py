#!/usr/bin/env python3
"""Cost of the reduced outputs of a resident column (want_M = edges / tiles) on one MI355X: tools/reduced_spectra_cost.py [--steps 30] [--rounds 3] [--parent-lib FILE] [--out profiles/reduced_spectra_cost.json]

The bench column (BASELINE configs[2], C3: H2O + CO2 line by line, 1e5 nu x 60 layers, Discretized(5, 2)), one resident column per case:
  none    want_M = False: band fluxes only
  planes  want_M = True: M+, M- [np, nnu], 98 MB
  edges   want_M = "edges": M+, M- at TOA and surface, [2, nnu], 3.2 MB
  tiles   want_M = "tiles": sums of w_j M over 64-point tiles, [np, ntile], 1.5 MB
Two figures per case, host wall clock: run + sync, and run + sync + fetch (the case's M outputs and the band fluxes into host arrays
allocated once).  The cases' steps are interleaved (step s of every case before step s + 1 of any), medians after 3 warm-up steps.

A measurement runs in a child process -- one per library -- so that --parent-lib FILE (the parent commit's library, built beforehand from
a checkout of that commit; the convention of tools/ab_lib.sh: the other build is a file named by path) is timed by the same code on the
same column: its none and planes cases.  Children of the two builds alternate for --rounds rounds; a case's spread is that of its round
medians, and a ratio between builds is formed round by round (neighbouring children) before its median is taken."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"none": False, "planes": True, "edges": "edges", "tiles": "tiles"}


def child(lib_path, cases, steps, warmup=3):
    import clearsky_jl_amd as cs
    if lib_path:
        cs._lib.LIB_PATH = lib_path            # (before the first call: lib() loads what this names)
    import workloads as W
    cfg = W.config("C3")
    cols, bufs = {}, {}
    for k in cases:
        ctx = cs.Context(0)
        col = cs.Column(cfg["P"], cfg["g"], cfg["T"], cfg["mu"], cfg["fS"], cfg["fa"], *cfg["absorbers"], core=cfg["core"], ctx=ctx,
                        want_tau=False, want_M=MODES[k])
        shape = {"planes": (col.np, col.nnu), "edges": (2, col.nnu), "tiles": (col.np, -(-col.nnu // 64))}.get(k)
        cols[k] = (ctx, col)
        bufs[k] = None if shape is None else (np.zeros(shape, order="F"), np.zeros(shape, order="F"))

    def step(k, fetch):
        col = cols[k][1]
        t0 = time.perf_counter()
        col.run()
        col.sync()
        if fetch:
            if bufs[k] is None:
                col.fetch()
            else:
                col.fetch(Mup=bufs[k][0], Mdn=bufs[k][1])
        return (time.perf_counter() - t0) * 1e3

    t = {k: {"run": [], "fetch": []} for k in cases}
    for s in range(warmup + steps):
        for fetch in (False, True):
            for k in cases:
                ms = step(k, fetch)
                if s >= warmup:
                    t[k]["fetch" if fetch else "run"].append(ms)
    out = {"build_id": cs.lib().cs_build_id().decode()}
    for k in cases:
        col = cols[k][1]
        Fup = col.fetch()[0]
        out[k] = dict(run_ms=float(np.median(t[k]["run"])), run_min_ms=float(np.min(t[k]["run"])), run_max_ms=float(np.max(t[k]["run"])),
                      run_fetch_ms=float(np.median(t[k]["fetch"])), run_fetch_min_ms=float(np.min(t[k]["fetch"])),
                      run_fetch_max_ms=float(np.max(t[k]["fetch"])), flux_form=col.info()["flux_form"], launches=col.info()["launches"],
                      Fup_toa=float(Fup[0]), M_bytes=0 if bufs[k] is None else int(2 * bufs[k][0].nbytes))
    for ctx, _ in cols.values():
        ctx.close()
    print("RESULT " + json.dumps(out))


def spawn(lib_path, cases, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", ",".join(cases), "--steps", str(steps)] + (["--lib", lib_path] if lib_path else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
    for ln in p.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    raise RuntimeError(f"child failed ({p.returncode}): {p.stderr[-2000:]}")


def summary(rounds, case):
    run = [r[case]["run_ms"] for r in rounds]
    fet = [r[case]["run_fetch_ms"] for r in rounds]
    return dict(run_ms=float(np.median(run)), run_round_medians_ms=run, run_spread_ms=float(np.max(run) - np.min(run)),
                run_fetch_ms=float(np.median(fet)), run_fetch_round_medians_ms=fet, run_fetch_spread_ms=float(np.max(fet) - np.min(fet)),
                flux_form=rounds[0][case]["flux_form"], launches=rounds[0][case]["launches"], Fup_toa=rounds[0][case]["Fup_toa"],
                M_bytes=rounds[0][case]["M_bytes"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduced_spectra_cost.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.lib, a.child.split(","), a.steps)
        return
    this, parent = [], []
    for _ in range(a.rounds):
        this.append(spawn(None, list(MODES), a.steps))
        if a.parent_lib:
            parent.append(spawn(os.path.abspath(a.parent_lib), ["none", "planes"], a.steps))
    out = {"what": __doc__.splitlines()[0], "column": "C3 (BASELINE configs[2]): 1e5 nu x 60 layers, H2O + CO2 line by line, Discretized(5, 2)",
           "steps": a.steps, "rounds": a.rounds, "build_id": this[0]["build_id"], "this": {k: summary(this, k) for k in MODES}}
    T = out["this"]

    def ratio(num, den, key):       # round by round, then the median and the range
        r = [x[num[1]][key] / y[den[1]][key] for x, y in zip(num[0], den[0])]
        return dict(median=float(np.median(r)), min=float(np.min(r)), max=float(np.max(r)))

    out["ratios"] = {
        "edges_run_vs_planes_run": ratio((this, "edges"), (this, "planes"), "run_ms"),
        "tiles_run_vs_planes_run": ratio((this, "tiles"), (this, "planes"), "run_ms"),
        "edges_run_vs_none_run": ratio((this, "edges"), (this, "none"), "run_ms"),
        "tiles_run_vs_none_run": ratio((this, "tiles"), (this, "none"), "run_ms"),
        "edges_run_fetch_vs_planes_run_fetch": ratio((this, "edges"), (this, "planes"), "run_fetch_ms"),
        "tiles_run_fetch_vs_planes_run_fetch": ratio((this, "tiles"), (this, "planes"), "run_fetch_ms"),
    }
    for k in ("planes", "edges", "tiles"):
        out["this"][k]["fetch_alone_ms"] = T[k]["run_fetch_ms"] - T[k]["run_ms"]
    if parent:
        out["parent_build_id"] = parent[0]["build_id"]
        out["parent"] = {k: summary(parent, k) for k in ("none", "planes")}
        for k in ("none", "planes"):
            out["ratios"][f"{k}_run_vs_parent"] = ratio((this, k), (parent, k), "run_ms")
            out["ratios"][f"{k}_run_fetch_vs_parent"] = ratio((this, k), (parent, k), "run_fetch_ms")
            assert T[k]["Fup_toa"] == out["parent"][k]["Fup_toa"], "the two builds disagree on the OLR"
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
