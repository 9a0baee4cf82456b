#!/usr/bin/env python
"""Timing of pagoda.top.aspects (scde_amd/top_aspects.py, scde_amd/rmt.py, csrc/top_aspects.hip).

    python tools/bench_top_aspects.py [--out profiles/top_aspects_bench.json]
                                      [--cases 200x2x100,5000x1x3000] [--reps 3] [--warmup 1] [--no-baseline]

Per case (gene sets x components x cells; a synthetic pwpca whose PC variances lie in the bulk of
the Tracy-Widom law, every tenth set 20 scalings above its centre), host -> host wall times, a
warm-up and then the median of --reps:

  * table     top_aspects_table with n_cells given: host statistics only, one Tracy-Widom
              evaluation per row plus three quantiles
  * device    the matrix step on every row of the case (scde_top_aspects: upload of scores and
              weights, one launch, xv and xvw back), and the kernel's own time from the context's
              HIP events.  Achieved bytes per second are the bytes the step must move -- scores
              and weights read once, xv and xvw written once, 32 per element -- over the kernel's
              time, beside a device-to-device copy of 1 GiB timed in the same run.

and once per run the Tracy-Widom evaluations per second on 200 points of [-4, 10].

The baseline is tests/top_aspects_ref.py, the float64 numpy / scipy restatement (its law from
eigvalsh on 128 nodes), on one CPU thread, timed once per case.  No ratio is expected in
advance; a stage slower than numpy is reported as such.  Prints one JSON document and writes it
to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"   # the baseline is one CPU thread

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_varnorm import _kernel_ms, _median_ms, copy_rate  # noqa: E402  (tools/ is on the path as the script's directory)


def synthetic_pwpca(nsets, ncomp, cells, seed=1):
    from scde_amd import rmt
    rng = np.random.default_rng(seed)
    sizes = rng.integers(10, 400, size=nsets)
    par = rmt.wishart_max_par(float(cells), sizes.astype(np.float64))
    pw = {}
    for j in range(nsets):
        # the scaled statistic: the bulk of the law, and 20 for every tenth set (the float64
        # restatement holds from -4 to where its matrix underflows)
        u = rng.uniform(-3.0, 3.0, size=ncomp)
        if j % 10 == 0:
            u[0] = 20.0
        var = par["centering"][j] + par["scaling"][j] * u
        xp = {"scores": rng.normal(size=(cells, ncomp)), "scoreweights": rng.uniform(0.2, 1.0, size=(cells, ncomp)),
              "rotation": rng.normal(size=(int(sizes[j]), ncomp)),
              "rotation_names": [f"g{(j * 7 + k) % 20000}" for k in range(int(sizes[j]))]}
        pw[f"set{j}"] = {"xp": xp, "sd": np.sqrt(var)[None, :], "n": int(sizes[j]), "z": np.ones((1, 1))}
    return pw


def bench_case(nsets, ncomp, cells, reps, warmup, baseline):
    import top_aspects_ref as R
    from scde_amd import api
    from scde_amd import top_aspects as T
    pw = synthetic_pwpca(nsets, ncomp, cells)
    ctx = api.default_context()
    keep = {}

    def table():
        keep["t"] = T.top_aspects_table(pw, n_cells=cells)

    r = {"rows": nsets * ncomp, "table_ms": _median_ms(table, reps, warmup)}
    t = keep["t"]
    r["valid_rows"] = int(t["valid"].sum())
    print(f"{nsets}x{ncomp}x{cells}: table {r['table_ms']:.1f} ms", flush=True)
    m = nsets * ncomp
    x = np.ascontiguousarray(np.concatenate([e["xp"]["scores"].T for e in pw.values()]))
    w = np.ascontiguousarray(np.concatenate([e["xp"]["scoreweights"].T for e in pw.values()]))
    num = np.ascontiguousarray(np.where(np.isfinite(t["score"]), t["score"], 1.0))

    def device():
        keep["d"] = T._scale_rows_dev(x, w, num, ctx)

    r["device_ms"] = _median_ms(device, reps, warmup)
    k = _kernel_ms(ctx, device, reps)
    nbytes = 32.0 * m * cells
    r.update(device_kernel_ms=k, device_bytes=nbytes, device_bytes_per_s=nbytes / (k * 1e-3) if k > 0 else None)
    print(f"{nsets}x{ncomp}x{cells}: device {r['device_ms']:.1f} ms, kernel {k:.3f} ms", flush=True)
    if baseline:
        t0 = time.perf_counter()
        rt = R.table(pw, float(cells))
        t1 = time.perf_counter()
        rxv, rxvw = R.scale_rows(x, w, num)
        t2 = time.perf_counter()
        r["numpy"] = {"table_ms": (t1 - t0) * 1e3, "device_ms": (t2 - t1) * 1e3}
        r["numpy_over_library"] = {k_: r["numpy"][k_ + "_ms"] / r[k_ + "_ms"] for k_ in ("table", "device")}
        ok = np.isfinite(rt["z"]) & np.isfinite(t["z"])
        r["max_abs_difference_z"] = float(np.max(np.abs(rt["z"][ok] - t["z"][ok])))
        r["max_abs_difference_xv"] = float(np.nanmax(np.abs(keep["d"][0] - rxv)))
    return r


def tw_rate(baseline):
    import top_aspects_ref as R
    from scde_amd import rmt
    s = np.linspace(-4.0, 10.0, 200)
    rmt.ptw_upper_log(s[:3])
    t0 = time.perf_counter()
    a = rmt.ptw_upper_log(s)
    t1 = time.perf_counter()
    out = {"points": len(s), "evaluations_per_s": len(s) / (t1 - t0)}
    if baseline:
        t0 = time.perf_counter()
        b = R.ptw_upper_log64(s)
        t1 = time.perf_counter()
        out["numpy_evaluations_per_s"] = len(s) / (t1 - t0)
        out["max_rel_difference"] = float(np.max(np.abs(a / b - 1.0)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="200x2x100,5000x1x3000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_aspects_bench.json"))
    args = ap.parse_args()
    doc = {"tool": "tools/bench_top_aspects.py", "reps": args.reps, "warmup": args.warmup,
           "device_copy_bytes_per_s": copy_rate(), "tracy_widom": tw_rate(not args.no_baseline), "cases": {}}
    print("tracy_widom", json.dumps(doc["tracy_widom"]), flush=True)
    for case in args.cases.split(","):
        nsets, ncomp, cells = (int(v) for v in case.split("x"))
        doc["cases"][case] = bench_case(nsets, ncomp, cells, args.reps, args.warmup, not args.no_baseline)
        print(case, json.dumps(doc["cases"][case]), flush=True)
    for c in doc["cases"].values():
        if isinstance(doc["device_copy_bytes_per_s"], float) and c["device_bytes_per_s"]:
            c["device_share_of_copy_rate"] = c["device_bytes_per_s"] / doc["device_copy_bytes_per_s"]
    txt = json.dumps(doc, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
