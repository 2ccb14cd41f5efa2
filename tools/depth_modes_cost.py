#!/usr/bin/env python3
"""Cost of the optical-depth modes of a resident column (want_tau = total / tiles) on one MI355X: tools/depth_modes_cost.py [--steps 30] [--rounds 3] [--parent-lib FILE] [--kernel-stats total=CSV,tiles=CSV] [--out profiles/depth_modes_cost.json]

The bench column (BASELINE configs[2], C3: H2O + CO2 line by line, 1e5 nu x 60 layers, Discretized(5, 2)), one resident column per case,
want_M = False in all four:
  none    want_tau = False
  layers  want_tau = True: the layer depths [np-1, nnu], 48 MB
  total   want_tau = "total": the slant optical depth of the column, [nnu], 0.8 MB; flux form 0 and k_depth
  tiles   want_tau = "tiles": sums of w_j exp(-D_i) over 64-point tiles, [np, ntile], 0.76 MB; flux form 0 and k_depth
Host wall clock of run + sync; the cases' steps are interleaved (step s of every case before step s + 1 of any), medians after 3 warm-up
steps.  Then opticaldepth on the same column's inputs (theta = the column's theta_s, nlobatto = its core's), wall clock of the whole call,
--od-reps times after one warm-up call: with this library cs.opticaldepth (a total column, sigma_run, nnu doubles back); with the parent's
the formula its package evaluated (the [nnu, K] plane fetched, the Lobatto sum in numpy: `opticaldepth_host` below).

A measurement runs in a child process -- one per library -- so that --parent-lib FILE (the parent commit's library, built beforehand from
a checkout of that commit; the convention of tools/ab_lib.sh: the other build is a file named by path) is timed by the same code on the
same column, in the same order: its none and layers cases, its opticaldepth.  Children of the two builds alternate for --rounds rounds; a
ratio between builds is formed round by round (neighbouring children) before its median is taken.

k_depth alone is not timed here: --trace MODE runs a total or a tiles column for --steps steps and nothing else, for a run of its own under
`rocprofv3 --kernel-trace --stats`; --kernel-stats names the kernel_stats CSV files of those runs and the JSON then holds k_depth's
average time next to the bytes it must move -- K nnu 8 B per plane read (two where the step keeps the near-line pairs apart) plus its
output -- and the rate that gives, beside the 6.3 TB/s a streaming kernel achieves on this part (8 TB/s specified)."""
import argparse
import csv
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"none": False, "layers": True, "total": "total", "tiles": "tiles"}
HBM_ACHIEVABLE_TBS = 6.3


def _column(cs, cfg, ctx, want_tau):
    return cs.Column(cfg["P"], cfg["g"], cfg["T"], cfg["mu"], cfg["fS"], cfg["fa"], *cfg["absorbers"], core=cfg["core"], ctx=ctx,
                     want_tau=want_tau, want_M=False)


def opticaldepth_host(cs, P, g, T, mu, theta, *absorbers, nlobatto=4, ctx=None):
    """opticaldepth as the package formed it before k_depth: the node cross-sections fetched, the Lobatto sum on the host"""
    P = np.sort(np.asarray(P, float))
    col = cs.Column(P, g, T, mu, None, None, *absorbers, core=cs.Discretized(5, nlobatto), want_tau=False, want_M=False, ctx=ctx)
    col.sigma_run()
    sig = col.sigma_nodes()
    Cc = 1e-4 * cs.constants.Na / g
    _, ws = cs.lobattonodes(nlobatto)
    m = 1 / math.cos(theta)
    beta = Cc * (sig / col.muk[:, None])
    tau = np.zeros(col.nnu)
    for i in range(len(P) - 1):
        dP = P[i + 1] - P[i]
        ti = np.zeros(col.nnu)
        for n in range(nlobatto):
            ti = ti + (dP * ws[n]) * beta[i * (nlobatto - 1) + n]
        tau = tau + ti * m
    return tau


def child(lib_path, cases, steps, od_reps, warmup=3):
    import clearsky_jl_amd as cs
    if lib_path:
        cs._lib.LIB_PATH = lib_path            # (before the first call: lib() loads what this names)
    import workloads as W
    cfg = W.config("C3")
    cols = {}
    for k in cases:
        ctx = cs.Context(0)
        cols[k] = (ctx, _column(cs, cfg, ctx, MODES[k]))
    t = {k: [] for k in cases}
    for s in range(warmup + steps):
        for k in cases:
            col = cols[k][1]
            t0 = time.perf_counter()
            col.run()
            col.sync()
            if s >= warmup:
                t[k].append((time.perf_counter() - t0) * 1e3)
    out = {"build_id": cs.lib().cs_build_id().decode()}
    for k in cases:
        col = cols[k][1]
        out[k] = dict(run_ms=float(np.median(t[k])), run_min_ms=float(np.min(t[k])), run_max_ms=float(np.max(t[k])),
                      flux_form=col.info()["flux_form"], launches=col.info()["launches"], near_plane_apart=bool(col.work()["dispatch"]["streams"] & 2),
                      Fup_toa=float(col.fetch()[0][0]), K=col.K, nnu=col.nnu, np=col.np)
    theta, nlob = cols[cases[0]][1].theta_s, cfg["core"].nlobatto
    for ctx, _ in cols.values():
        ctx.close()
    ctx = cs.Context(0)
    od = cs.opticaldepth if "total" in cases else (lambda *a, **kw: opticaldepth_host(cs, *a, **kw))
    ts = []
    for r in range(od_reps + 1):
        t0 = time.perf_counter()
        D = od(cfg["P"], cfg["g"], cfg["T"], cfg["mu"], theta, *cfg["absorbers"], nlobatto=nlob, ctx=ctx)
        if r:
            ts.append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    out["opticaldepth"] = dict(wall_ms=float(np.median(ts)), wall_min_ms=float(np.min(ts)), wall_max_ms=float(np.max(ts)), reps=od_reps,
                               D_min=float(D.min()), D_max=float(D.max()), D_sum=float(math.fsum(D)))
    print("RESULT " + json.dumps(out))


def trace(mode, steps):
    """a total or a tiles column run `steps` times and nothing else: the process rocprofv3 traces"""
    import clearsky_jl_amd as cs
    import workloads as W
    cfg = W.config("C3")
    ctx = cs.Context(0)
    col = _column(cs, cfg, ctx, mode)
    for _ in range(steps + 3):
        col.run()
        col.sync()
    ctx.close()


def spawn(lib_path, cases, steps, od_reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", ",".join(cases), "--steps", str(steps), "--od-reps", str(od_reps)]
    p = subprocess.run(cmd + (["--lib", lib_path] if lib_path else []), capture_output=True, text=True, timeout=280)
    for ln in p.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    raise RuntimeError(f"child failed ({p.returncode}): {p.stderr[-2000:]}")


def summary(rounds, case):
    run = [r[case]["run_ms"] for r in rounds]
    d = dict(rounds[0][case])
    d.update(run_ms=float(np.median(run)), run_round_medians_ms=run, run_spread_ms=float(np.max(run) - np.min(run)))
    return d


def kernel_stats(path):
    """k_depth's row of a rocprofv3 kernel_stats CSV: calls, average and total time"""
    with open(path) as f:
        for row in csv.DictReader(f):
            if "k_depth" in row.get("Name", ""):
                return dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, total_us=float(row["TotalDurationNs"]) / 1e3,
                            min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
    raise RuntimeError(f"no k_depth row in {path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--od-reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernel-stats", default=None, help="total=FILE,tiles=FILE: kernel_stats CSVs of two --trace runs under rocprofv3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_modes_cost.json"))
    ap.add_argument("--trace", default=None, choices=["total", "tiles"])
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace:
        trace(a.trace, a.steps)
        return
    if a.child:
        child(a.lib, a.child.split(","), a.steps, a.od_reps)
        return
    this, parent = [], []
    for _ in range(a.rounds):
        this.append(spawn(None, list(MODES), a.steps, a.od_reps))
        if a.parent_lib:
            parent.append(spawn(os.path.abspath(a.parent_lib), ["none", "layers"], a.steps, a.od_reps))
    out = {"what": __doc__.splitlines()[0], "column": "C3 (BASELINE configs[2]): 1e5 nu x 60 layers, H2O + CO2 line by line, Discretized(5, 2)",
           "steps": a.steps, "rounds": a.rounds, "build_id": this[0]["build_id"], "this": {k: summary(this, k) for k in MODES}}
    T = out["this"]

    def ratio(num, den, f):       # round by round, then the median and the range
        r = [f(x[num[1]]) / f(y[den[1]]) for x, y in zip(num[0], den[0])]
        return dict(median=float(np.median(r)), min=float(np.min(r)), max=float(np.max(r)))

    run = lambda d: d["run_ms"]
    out["ratios"] = {f"{k}_run_vs_none_run": ratio((this, k), (this, "none"), run) for k in ("layers", "total", "tiles")}
    od = [r["opticaldepth"] for r in this]
    out["this"]["opticaldepth"] = dict(od[0], wall_ms=float(np.median([o["wall_ms"] for o in od])), wall_round_medians_ms=[o["wall_ms"] for o in od])
    if parent:
        out["parent_build_id"] = parent[0]["build_id"]
        out["parent"] = {k: summary(parent, k) for k in ("none", "layers")}
        for k in ("none", "layers"):
            out["ratios"][f"{k}_run_vs_parent"] = ratio((this, k), (parent, k), run)
            assert T[k]["Fup_toa"] == out["parent"][k]["Fup_toa"], "the two builds disagree on the OLR"
        pod = [r["opticaldepth"] for r in parent]
        out["parent"]["opticaldepth"] = dict(pod[0], wall_ms=float(np.median([o["wall_ms"] for o in pod])), wall_round_medians_ms=[o["wall_ms"] for o in pod])
        out["ratios"]["opticaldepth_wall_vs_parent"] = ratio((this, "opticaldepth"), (parent, "opticaldepth"), lambda d: d["wall_ms"])
        out["opticaldepth_sum_rel_diff_vs_parent"] = abs(od[0]["D_sum"] - pod[0]["D_sum"]) / pod[0]["D_sum"]
    if a.kernel_stats:
        out["k_depth"] = {}
        for item in a.kernel_stats.split(","):
            mode, path = item.split("=", 1)
            c = T[mode]
            planes = 2 if c["near_plane_apart"] else 1
            nbytes = planes * c["K"] * c["nnu"] * 8 + (c["nnu"] if mode == "total" else c["np"] * -(-c["nnu"] // 64)) * 8 + (c["nnu"] * 8 if mode == "tiles" else 0)
            ks = kernel_stats(path)
            out["k_depth"][mode] = dict(ks, planes_read=planes, bytes=nbytes, tb_per_s=nbytes / (ks["average_us"] * 1e-6) / 1e12,
                                        achievable_tb_per_s=HBM_ACHIEVABLE_TBS)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
