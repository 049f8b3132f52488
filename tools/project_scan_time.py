#!/usr/bin/env python3
"""Time the projected scan (sfs2d_plan_project_scan: k_proj_win over the chromosome, k_proj_lp, k_proj_scan) beside
k_proj_win with every window its own group over the same windows.

Section 18's setup: one synthetic chromosome of 1,562,500 SNPs (synth_genome seed 777, missing alleles at 2 %), a
counts plan with per-chromosome background at 20 kb, 4,362 windows.  A configuration is (diploids of population 1,
of population 2, m1, m2); the default list is 25 + 25 diploids at (40, 40) and 18 / 14 at (24, 20).  k_proj_win over
every window as its own group evaluates the same weights into the same LDS grids and flushes each grid to its row in
global memory, where k_proj_scan reduces it in place: the yardstick.  Cases, both into a caller's device buffer:

  each  sfs2d_plan_project, every window its own group (one k_proj_win dispatch)
  scan  sfs2d_plan_project_scan (k_proj_win over the chromosome entry's pieces, k_proj_lp, k_proj_scan)

  run        per configuration one warm-up repetition, then `rounds` x `reps` repetitions of [each, scan] interleaved
             -- meant to run under `rocprofv3 --kernel-trace --output-format csv`, which times every dispatch; then,
             per case, the whole call between two events on the stream, `rounds` times `reps` calls.  Prints one JSON
             line per configuration.
  summarise  the kernel-trace CSV of such a run: the dispatches in start order are dealt to the configurations and
             cases by the fixed order (per repetition: k_proj_win of `each`, then k_proj_win, k_proj_lp and k_proj_scan
             of `scan`), the warm-ups dropped, cut into `rounds` groups; each group's mean, and the median / min / max
             of the groups.  One JSON line per configuration.

usage: rocprofv3 --kernel-trace --output-format csv -d OUT -o pscan -- python tools/project_scan_time.py run
       python tools/project_scan_time.py summarise OUT/.../pscan_kernel_trace.csv"""
import argparse
import csv
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2dsfs-scan_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["run", "summarise"])
ap.add_argument("trace", nargs="?")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
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
    win, lp, scan = [], [], []
    for r in sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"])):
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        for name, v in (("k_proj_win", win), ("k_proj_lp", lp), ("k_proj_scan", scan)):
            if name in r["Kernel_Name"]:
                v.append(us)
    R = a.rounds * a.reps
    # a configuration's dispatches: the interleaved repetitions (warm-up first), then the event-timed calls, R per
    # case, and one read-back call of `scan` -- skipped here
    nw, ns = 2 * (R + 1) + 2 * R + 1, (R + 1) + R + 1
    for i, cfg in enumerate(CONFIGS):
        w, out = win[nw * i:nw * i + 2 * (R + 1)], {"diploids": cfg[:2], "project": cfg[2:]}
        out["each_k_proj_win"] = groups(w[0::2][1:], a.rounds)
        out["scan_k_proj_win_chromosome"] = groups(w[1::2][1:], a.rounds)
        out["scan_k_proj_lp"] = groups(lp[ns * i:ns * i + R + 1][1:], a.rounds)
        out["scan_k_proj_scan"] = groups(scan[ns * i:ns * i + R + 1][1:], a.rounds)
        if out["each_k_proj_win"] and out["scan_k_proj_scan"]:
            out["k_proj_scan_over_each"] = round(out["scan_k_proj_scan"]["us"] / out["each_k_proj_win"]["us"], 3)
        print(json.dumps(out))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sfs2d import _lib as L  # noqa: E402
from sfs2d.engine import Engine, ScanConfig  # noqa: E402
from sfs2d.synth import synth_genome  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("project_scan_time: no GPU (timings are taken on the device only)")
eng = Engine.get(0)
stream = torch.cuda.Stream()
eng.set_stream(stream.cuda_stream)


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
    pbuf = torch.empty(pl.nrec * L.proj_row_words(m1, m2), dtype=torch.int64, device="cuda")
    sbuf = torch.empty(pl.nrec * 8, dtype=torch.int64, device="cuda")
    cases = {"each": lambda: pl.project(m1, m2, out_dev_ptr=pbuf.data_ptr()),
             "scan": lambda: pl.project_scan(m1, m2, out_dev_ptr=sbuf.data_ptr())}
    for fn in cases.values():   # the warm-up repetition
        fn()
    stream.synchronize()
    for _ in range(a.rounds):
        for _ in range(a.reps):
            for fn in cases.values():
                fn()
        stream.synchronize()
    pl.check()
    out = {"snps": p.n, "diploids": [n1p, n2p], "project": [m1, m2], "window": 20000, "records": int(pl.nrec),
           "rounds": a.rounds, "reps": a.reps, "call_us": {}}
    for k, fn in cases.items():
        v = [event_us(fn, a.reps) for _ in range(a.rounds)]
        out["call_us"][k] = {"us": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
    st = pl.project_scan(m1, m2)
    out.update(e=pl.project_scan_e, e_bg=pl.project_scan_e_bg, n_used=int(st["n_used"].sum()),
               n_dropped=int(st["n_dropped"].sum()), finite_t2d=int(np.isfinite(st["t2d"]).sum()),
               median_t2d=float(np.nanmedian(st["t2d"])))
    print(json.dumps(out), flush=True)
    del pbuf, sbuf
    pl.close()
    dev.close()
