#!/usr/bin/env python3
"""Time k_spec_win (sfs2d_plan_spectra) beside k_div_win over the same windows.

DESIGN.md section 15's setup: one synthetic chromosome of 1,562,500 SNPs (synth_genome seed 777, 25 + 25 diploids:
a 51 x 51 grid), a counts plan with per-chromosome background at 20 kb, 4,362 windows.  k_div_win reads the same
4 B/SNP over the same windows and is the yardstick.  Cases, all into a caller's device buffer:

  a   every window, each its own group (the per-window export);
  a1  the same windows pooled into one group (what (a) spends on its per-window flushes is a - a1);
  b   the top 1 % of the windows by T2D pooled into one group;
  c   DESIGN.md section 16's case (c): 20,000 gene-like regions (log-uniform 1 kb - 1 Mb) of the 1e6-SNP chromosome
      (seed 12345), each its own group; c1: the same regions pooled into one group.

  run        one warm-up repetition, then `rounds` x `reps` repetitions of [diversity, a, a1, b] interleaved, then
             one warm-up and `rounds` x `creps` repetitions of [c, c1] -- meant to run under
             `rocprofv3 --kernel-trace --output-format csv`, which times every dispatch; then, per case, the whole
             call (the rows' memset, the selection's copy, the kernel) between two events on the stream, `rounds`
             times `reps` calls.  Prints one JSON line with the event timings.
  summarise  the kernel-trace CSV of such a run: the k_spec_win dispatches in start order are dealt to the cases by
             the repetition's fixed order, the warm-up dropped, cut into `rounds` groups; each group's mean, and the
             median / min / max of the groups.  One JSON line.

usage: rocprofv3 --kernel-trace --output-format csv -d OUT -o spec -- python tools/spectra_time.py run
       python tools/spectra_time.py summarise OUT/.../spec_kernel_trace.csv"""
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
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--creps", type=int, default=4)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--snps", type=int, default=1_562_500)
a = ap.parse_args()


def groups(v, rounds):
    n = len(v) // rounds
    g = [statistics.mean(v[i * n:(i + 1) * n]) for i in range(rounds)] if n else []
    if not g:
        return None
    return {"dispatches": len(v), "round_means_us": [round(x, 2) for x in g], "us": round(statistics.median(g), 2),
            "us_min": round(min(g), 2), "us_max": round(max(g), 2), "fastest_dispatch_us": round(min(v), 2)}


if a.mode == "summarise":
    div, spec = [], []
    for r in sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"])):
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "k_div_win" in r["Kernel_Name"]:
            div.append(us)
        elif "k_spec_win" in r["Kernel_Name"]:
            spec.append(us)
    R, C = a.rounds * a.reps, a.rounds * a.creps
    first, second = spec[:3 * (R + 1)], spec[3 * (R + 1):3 * (R + 1) + 2 * (C + 1)]
    out = {"k_div_win": groups(div[1:R + 1], a.rounds)}
    for k, name in enumerate(("a_each_window", "a1_same_windows_one_group", "b_top_1pct_one_group")):
        out[name] = groups(first[k::3][1:], a.rounds)
    for k, name in enumerate(("c_each_region", "c1_same_regions_one_group")):
        out[name] = groups(second[k::2][1:], a.rounds)
    if out["k_div_win"] and out["a_each_window"]:
        out["a_over_div"] = round(out["a_each_window"]["us"] / out["k_div_win"]["us"], 3)
        out["a_flush_share"] = round(1.0 - out["a1_same_windows_one_group"]["us"] / out["a_each_window"]["us"], 3)
    print(json.dumps(out))
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sfs2d import _lib as L  # noqa: E402
from sfs2d.engine import Engine, ScanConfig  # noqa: E402
from sfs2d.regions import Regions, region_ranges  # noqa: E402
from sfs2d.synth import synth_genome  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("spectra_time: no GPU (timings are taken on the device only)")
eng = Engine.get(0)
stream = torch.cuda.Stream()
eng.set_stream(stream.cuda_stream)
roww = L.spec_row_words(25, 25)

p = synth_genome(1, a.snps, 25, 25, seed=777)
dev = eng.upload(p)
pl = eng.plan(dev, ScanConfig(n1p=25, n2p=25, window=20000, bg_mode=L.BG_PER_CHROM))
pl.run()
pl.check()
recs = pl.read()
live = np.nonzero((recs["flags"] & (L.W_EMPTY | L.W_EXTRA)) == 0)[0]
t2d = recs["t2d"][live]
top = live[t2d >= np.quantile(t2d[np.isfinite(t2d)], 0.99, method="higher")]
dbuf = torch.empty(pl.nrec * L.DIVERSITY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
sbuf = torch.empty(pl.nrec * roww, dtype=torch.int64, device="cuda")
zeros = np.zeros(pl.nrec, np.int32)
cases = {"diversity": lambda: pl.diversity(out_dev_ptr=dbuf.data_ptr()),
         "a_each_window": lambda: pl.spectra(out_dev_ptr=sbuf.data_ptr()),
         "a1_same_windows_one_group": lambda: pl.spectra(None, zeros, 1, out_dev_ptr=sbuf.data_ptr()),
         "b_top_1pct_one_group": lambda: pl.spectra(top, zeros[:len(top)], 1, out_dev_ptr=sbuf.data_ptr())}

q = synth_genome(1, 1_000_000, 25, 25, seed=12345)
name, last = q.chrom_names[0], int(q.pos[-1])
rng = np.random.Generator(np.random.PCG64(16))
length = np.exp(rng.uniform(np.log(1e3), np.log(1e6), size=20_000)).astype(np.int64)
first = 1 + (rng.random(20_000) * np.maximum(1, last - length)).astype(np.int64)
genes = Regions(q.chrom_names, [(name, int(f), int(f + n - 1), f"g{i}") for i, (f, n) in enumerate(zip(first, length))])
qdev = eng.upload(q)
rp = eng.plan(qdev, ScanConfig(n1p=25, n2p=25, bg_mode=L.BG_PER_CHROM, regions=genes))
rp.run()
rp.check()
cbuf = torch.empty(rp.nrec * roww, dtype=torch.int64, device="cuda")
czeros = np.zeros(rp.nrec, np.int32)
ccases = {"c_each_region": lambda: rp.spectra(out_dev_ptr=cbuf.data_ptr()),
          "c1_same_regions_one_group": lambda: rp.spectra(None, czeros, 1, out_dev_ptr=cbuf.data_ptr())}

for group, reps in ((cases, a.reps), (ccases, a.creps)):
    for fn in group.values():   # the warm-up repetition
        fn()
    stream.synchronize()
    for _ in range(a.rounds):
        for _ in range(reps):
            for fn in group.values():
                fn()
        stream.synchronize()
pl.check()
rp.check()


def event_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


b, e = region_ranges(q, genes)
out = {"snps": p.n, "grid": [51, 51], "window": 20000, "records": int(pl.nrec), "windows": int(len(live)),
       "top_1pct_windows": int(len(top)), "row_words": roww, "rounds": a.rounds, "reps": a.reps, "creps": a.creps,
       "c_snps": q.n, "c_regions": int(rp.nrec), "c_snps_scanned": int((e - b).sum()), "c_snps_per_region_max": int((e - b).max()),
       "call_us": {}}
for group, reps in ((cases, a.reps), (ccases, a.creps)):
    for k, fn in group.items():
        v = [event_us(fn, reps) for _ in range(a.rounds)]
        out["call_us"][k] = {"us": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
print(json.dumps(out))
rp.close()
qdev.close()
pl.close()
dev.close()
