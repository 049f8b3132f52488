#!/usr/bin/env python3
"""Time k_proj_win (sfs2d_plan_project) beside k_spec_win over the same windows.

DESIGN.md section 17's setup: one synthetic chromosome of 1,562,500 SNPs (synth_genome seed 777, missing alleles at
2 %), a counts plan with per-chromosome background at 20 kb, 4,362 windows.  k_spec_win streams the same 4 B/SNP over
the same windows and adds one 2D bin per SNP: the yardstick.  A configuration is (diploids per population, projection);
the default list is section 17's 25 + 25 diploids (a 51 x 51 grid) at (50, 50) and (40, 40), and the same generator at
50 + 50 diploids (101 x 101) at (100, 100) and (80, 80).  Cases per configuration, all into a caller's device buffer:

  spec_a  k_spec_win, every window its own group        spec_b  k_spec_win, the top 1 % of the windows by T2D pooled
  a       every window its own group                    b       the top 1 % pooled into one group
  c       one chromosome entry (the projected background)

  run        per configuration one warm-up repetition, then `rounds` x `reps` repetitions of [spec_a, spec_b, a, b, c]
             interleaved -- meant to run under `rocprofv3 --kernel-trace --output-format csv`, which times every
             dispatch; then, per case, the whole call (the rows' memset, the selection's copy, the kernel) between two
             events on the stream, `rounds` times `reps` calls.  Prints one JSON line per configuration.
  summarise  the kernel-trace CSV of such a run: the k_spec_win and k_proj_win dispatches in start order are dealt to
             the configurations and cases by the fixed order, the warm-ups dropped, cut into `rounds` groups; each
             group's mean, and the median / min / max of the groups.  One JSON line per configuration.

usage: rocprofv3 --kernel-trace --output-format csv -d OUT -o proj -- python tools/project_time.py run
       python tools/project_time.py summarise OUT/.../proj_kernel_trace.csv"""
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
ap.add_argument("--configs", default="25:50,25:40,50:100,50:80", help="DIPLOIDS:M, comma-separated (both populations alike)")
a = ap.parse_args()
CONFIGS = [tuple(int(x) for x in c.split(":")) for c in a.configs.split(",")]
SPEC, PROJ = ("spec_a", "spec_b"), ("a_each_window", "b_top_1pct_one_group", "c_one_chromosome_entry")


def groups(v, rounds):
    n = len(v) // rounds
    g = [statistics.mean(v[i * n:(i + 1) * n]) for i in range(rounds)] if n else []
    if not g:
        return None
    return {"dispatches": len(v), "round_means_us": [round(x, 2) for x in g], "us": round(statistics.median(g), 2),
            "us_min": round(min(g), 2), "us_max": round(max(g), 2), "fastest_dispatch_us": round(min(v), 2)}


if a.mode == "summarise":
    spec, proj = [], []
    for r in sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"])):
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "k_spec_win" in r["Kernel_Name"]:
            spec.append(us)
        elif "k_proj_win" in r["Kernel_Name"]:
            proj.append(us)
    R = a.rounds * a.reps
    # a configuration's dispatches: the interleaved repetitions (warm-up first), then one read-back call of case c
    # and the event-timed calls, R per case -- skipped here
    ns, nq = 2 * (R + 1) + 2 * R, 3 * (R + 1) + 1 + 3 * R
    for i, (npop, m) in enumerate(CONFIGS):
        s, q = spec[ns * i:ns * i + 2 * (R + 1)], proj[nq * i:nq * i + 3 * (R + 1)]
        out = {"diploids": npop, "project": [m, m]}
        for k, name in enumerate(SPEC):
            out[name] = groups(s[k::2][1:], a.rounds)
        for k, name in enumerate(PROJ):
            out[name] = groups(q[k::3][1:], a.rounds)
        if out["spec_a"] and out["a_each_window"]:
            out["a_over_spec_a"] = round(out["a_each_window"]["us"] / out["spec_a"]["us"], 2)
            out["b_over_spec_b"] = round(out["b_top_1pct_one_group"]["us"] / out["spec_b"]["us"], 2)
        print(json.dumps(out))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sfs2d import _lib as L  # noqa: E402
from sfs2d.engine import Engine, ScanConfig  # noqa: E402
from sfs2d.synth import synth_genome  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("project_time: no GPU (timings are taken on the device only)")
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


data = {}
for npop, m in CONFIGS:
    if npop not in data:
        for d in data.values():   # (one data set resident at a time)
            d[2].close()
            d[1].close()
        data.clear()
        p = synth_genome(1, a.snps, npop, npop, seed=777)
        dev = eng.upload(p)
        pl = eng.plan(dev, ScanConfig(n1p=npop, n2p=npop, window=20000, bg_mode=L.BG_PER_CHROM))
        pl.run()
        pl.check()
        data[npop] = (p, dev, pl)
    p, dev, pl = data[npop]
    recs = pl.read()
    live = np.nonzero((recs["flags"] & (L.W_EMPTY | L.W_EXTRA)) == 0)[0]
    t2d = recs["t2d"][live]
    top = live[t2d >= np.quantile(t2d[np.isfinite(t2d)], 0.99, method="higher")]
    sbuf = torch.empty(pl.nrec * L.spec_row_words(npop, npop), dtype=torch.int64, device="cuda")
    pbuf = torch.empty(pl.nrec * L.proj_row_words(m, m), dtype=torch.int64, device="cuda")
    zeros = np.zeros(pl.nrec, np.int32)
    cases = {"spec_a": lambda: pl.spectra(out_dev_ptr=sbuf.data_ptr()),
             "spec_b": lambda: pl.spectra(top, zeros[:len(top)], 1, out_dev_ptr=sbuf.data_ptr()),
             "a_each_window": lambda: pl.project(m, m, out_dev_ptr=pbuf.data_ptr()),
             "b_top_1pct_one_group": lambda: pl.project(m, m, top, zeros[:len(top)], 1, out_dev_ptr=pbuf.data_ptr()),
             "c_one_chromosome_entry": lambda: pl.project(m, m, [-1], [0], 1, out_dev_ptr=pbuf.data_ptr())}
    for fn in cases.values():   # the warm-up repetition
        fn()
    stream.synchronize()
    for _ in range(a.rounds):
        for _ in range(a.reps):
            for fn in cases.values():
                fn()
        stream.synchronize()
    pl.check()
    g, used, dropped = pl.project(m, m, [-1], [0], 1)
    out = {"snps": p.n, "diploids": npop, "project": [m, m], "window": 20000, "records": int(pl.nrec),
           "windows": int(len(live)), "top_1pct_windows": int(len(top)), "row_words": L.proj_row_words(m, m),
           "e_one_entry": pl.project_e, "chromosome_used": int(used[0]), "chromosome_dropped": int(dropped[0]),
           "grid_sum": float(g.sum()), "rounds": a.rounds, "reps": a.reps, "call_us": {}}
    for k, fn in cases.items():
        v = [event_us(fn, a.reps) for _ in range(a.rounds)]
        out["call_us"][k] = {"us": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
    print(json.dumps(out), flush=True)
    del sbuf, pbuf
for p, dev, pl in data.values():
    pl.close()
    dev.close()
