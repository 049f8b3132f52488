#!/usr/bin/env python3
"""Time the null of the projected scan (sfs2d_plan_project_null: the pool build once, then k_proj_null) beside the
projected scan's k_proj_scan over the same windows.

Section 19's setup: one synthetic chromosome of 1,562,500 SNPs (synth_genome seed 777, missing alleles at 2 %), a
counts plan with per-chromosome background at 20 kb, 4,362 windows.  A configuration is (diploids of population 1,
of population 2, m1, m2); the default list is 25 + 25 diploids at (40, 40) and 18 / 14 at (24, 20).  k_proj_scan's
time per record on those windows, in the same process and interleaved, is the yardstick for k_proj_null's time per
replicate record at R replicates (default 99): per slot the null adds half a Philox call and three dependent gathers
to the same walk and the same reduction.  Both into a caller's device buffer.

  run        per configuration the first project_null call alone (wall clock: it builds the pools -- the background
             rows and ln tables, the stratum keys, the stable radix sort, the segment heads -- and synchronises), then
             `rounds` x `reps` repetitions of [scan, null] interleaved -- meant to run under `rocprofv3 --kernel-trace
             --output-format csv`, which times every dispatch; then, per case, the whole call between two events on the
             stream, `rounds` times `reps` calls.  Prints one JSON line per configuration.
  summarise  the kernel-trace CSV of such a run: k_proj_scan's and k_proj_null's dispatches in start order dealt to
             the configurations by the fixed order, the warm-ups dropped, cut into `rounds` groups; each group's mean,
             the median / min / max of the groups, the time per record and the ratio; and the pool build's kernels
             (k_pnull_keys, the radix sort's, k_pnull_heads; one build per configuration), summed per configuration.

usage: rocprofv3 --kernel-trace --output-format csv -d OUT -o pnull -- python tools/project_null_time.py run
       python tools/project_null_time.py summarise OUT/.../pnull_kernel_trace.csv"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2dsfs-scan_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["run", "summarise"])
ap.add_argument("trace", nargs="?")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--replicates", type=int, default=99)
ap.add_argument("--records", type=int, default=4362, help="summarise: the plan's records (run prints them)")
ap.add_argument("--snps", type=int, default=1_562_500)
ap.add_argument("--configs", default="25:25:40:40,18:14:24:20", help="N1P:N2P:M1:M2, comma-separated")
a = ap.parse_args()
CONFIGS = [tuple(int(x) for x in c.split(":")) for c in a.configs.split(",")]


def groups(v, rounds):
    n = len(v) // rounds
    g = [statistics.mean(v[i * n:(i + 1) * n]) for i in range(rounds)] if n else []
    if not g:
        return None
    return {"dispatches": len(v), "round_means_us": [round(x, 2) for x in g], "us": round(statistics.median(g), 2),
            "us_min": round(min(g), 2), "us_max": round(max(g), 2), "fastest_dispatch_us": round(min(v), 2)}


if a.mode == "summarise":
    scan, null, build = [], [], []
    for r in sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"])):
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        name = r["Kernel_Name"]
        if "k_proj_scan" in name:
            scan.append(us)
        elif "k_proj_null" in name:
            null.append(us)
            build.append(None)      # (a mark: the build's kernels of a configuration come before its first k_proj_null)
        elif "k_pnull_" in name or "rocprim" in name:
            build.append((name.split("(")[0][-60:], us))
    R = a.rounds * a.reps
    # a configuration's dispatches per case: the cold call (null) / the warm-up (scan), the interleaved repetitions,
    # the event-timed calls, and for scan one read-back call -- the repetitions alone are kept
    ns, nn = 1 + R + R + 1, 1 + R + R
    # the pool builds: the runs of build kernels between k_proj_null marks that are not empty, one per configuration
    runs, cur = [], []
    for b in build:
        if b is None:
            if cur:
                runs.append(cur)
            cur = []
        else:
            cur.append(b)
    for i, cfg in enumerate(CONFIGS):
        out = {"diploids": cfg[:2], "project": cfg[2:], "replicates": a.replicates, "records": a.records}
        out["k_proj_scan"] = groups(scan[ns * i + 1:ns * i + 1 + R], a.rounds)
        out["k_proj_null"] = groups(null[nn * i + 1:nn * i + 1 + R], a.rounds)
        if out["k_proj_scan"] and out["k_proj_null"]:
            s = out["k_proj_scan"]["us"] / a.records
            n = out["k_proj_null"]["us"] / (a.records * a.replicates)
            out.update(k_proj_scan_ns_per_record=round(1e3 * s, 2), k_proj_null_ns_per_record=round(1e3 * n, 2),
                       null_over_scan_per_record=round(n / s, 3),
                       yardstick_spread=round(out["k_proj_scan"]["us_max"] / out["k_proj_scan"]["us_min"], 3))
        if i < len(runs):
            out["pool_build_kernels"] = len(runs[i])
            out["pool_build_us"] = round(sum(us for _, us in runs[i]), 2)
            out["pool_build_own_kernels_us"] = round(sum(us for n_, us in runs[i] if "k_pnull_" in n_), 2)
        print(json.dumps(out))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sfs2d import _lib as L  # noqa: E402
from sfs2d.engine import Engine, ScanConfig  # noqa: E402
from sfs2d.synth import synth_genome  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("project_null_time: no GPU (timings are taken on the device only)")
eng = Engine.get(0)
stream = torch.cuda.Stream()
eng.set_stream(stream.cuda_stream)
R = a.replicates


def event_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for n1p, n2p, m1, m2 in CONFIGS:
    p = synth_genome(1, a.snps, n1p, n2p, seed=777)
    dev = eng.upload(p)
    pl = eng.plan(dev, ScanConfig(n1p=n1p, n2p=n2p, window=20000, bg_mode=L.BG_PER_CHROM))
    pl.run()
    pl.check()
    sbuf = torch.empty(pl.nrec * 8, dtype=torch.int64, device="cuda")
    nbuf = torch.empty(pl.nrec * R * 8, dtype=torch.int64, device="cuda")
    cases = {"scan": lambda: pl.project_scan(m1, m2, out_dev_ptr=sbuf.data_ptr()),
             "null": lambda: pl.project_null(m1, m2, R, 1, out_dev_ptr=nbuf.data_ptr())}
    cases["scan"]()      # the warm-up repetition
    stream.synchronize()
    t0 = time.perf_counter()
    _, thin = cases["null"]()      # the cold call: the pool build, k_proj_null, the thin counts read back
    cold_ms = (time.perf_counter() - t0) * 1e3
    for _ in range(a.rounds):
        for _ in range(a.reps):
            for fn in cases.values():
                fn()
        stream.synchronize()
    pl.check()
    out = {"snps": p.n, "diploids": [n1p, n2p], "project": [m1, m2], "window": 20000, "records": int(pl.nrec),
           "replicates": R, "rounds": a.rounds, "reps": a.reps, "cold_call_ms": round(cold_ms, 2), "call_us": {}}
    for k, fn in cases.items():
        v = [event_us(fn, a.reps) for _ in range(a.rounds)]
        out["call_us"][k] = {"us": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
    st = pl.project_scan(m1, m2)
    nrec = np.frombuffer(nbuf.cpu().numpy().tobytes(), dtype=L.PROJSTAT_DTYPE)
    out.update(e=pl.project_null_e, e_bg=pl.project_null_e_bg, n_used=int(st["n_used"].sum()), thin_slots=int(thin.sum()),
               finite_t2d=int(np.isfinite(nrec["t2d"]).sum()), median_null_t2d=float(np.nanmedian(nrec["t2d"])),
               median_t2d=float(np.nanmedian(st["t2d"])))
    print(json.dumps(out), flush=True)
    del sbuf, nbuf
    pl.close()
    dev.close()
