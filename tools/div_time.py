#!/usr/bin/env python3
"""Time k_div_win (sfs2d_plan_diversity) beside k_fst_win over the same windows, and beside the plan's pass.

DESIGN.md section 14's chromosome: one synthetic chromosome of 1,562,500 SNPs (synth_genome, 25 + 25 diploids: a
51 x 51 grid), a counts plan with per-chromosome background at 20 kb.  Both kernels are a wavefront per window
over the same 4 B/SNP of packed counts, so k_fst_win is the yardstick.  The library launches k_fst_win on its own
for an Fst plan attached to a sliced base whose scan does not sum Fst (SFS2D_FST_SCAN=0 at plan creation); attached
at the base's own 20 kb, its windows are the ordinary plan's.

  run        `rounds` rounds of `reps` x (the base plan's run with its attached Fst plan, then the ordinary plan's diversity call),
             interleaved in one process -- meant to run under `rocprofv3 --kernel-trace --output-format csv`, which
             times every dispatch; prints one JSON line with what the host can time itself: the ordinary plan's
             whole pass (run_many, wall clock) and the diversity call between two events on the stream.
  summarise  the kernel-trace CSV of such a run: per kernel, the dispatches in start order cut into `rounds` equal
             groups (the warm-up dispatch and whatever follows the interleaved rounds dropped), each group's mean, and the median / min / max of the groups;
             bytes/s against the 4 B/SNP both kernels read.  One JSON line.

usage: rocprofv3 --kernel-trace --output-format csv -d OUT -o div -- python tools/div_time.py run [--reps 20] [--rounds 5]
       python tools/div_time.py summarise OUT/.../div_kernel_trace.csv [--reps 20] [--rounds 5]"""
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
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--snps", type=int, default=1_562_500)
a = ap.parse_args()

if a.mode == "summarise":
    per = {"k_div_win": [], "k_fst_win": []}
    for r in sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"])):
        for k in per:
            if k in r["Kernel_Name"]:
                per[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {"snps": a.snps, "bytes_per_call": 4 * a.snps}
    for k, v in per.items():
        v = v[1:1 + a.rounds * a.reps]   # after the warm-up dispatch, the interleaved ones (not the event-timed loop's)
        n = len(v) // a.rounds
        groups = [statistics.mean(v[i * n:(i + 1) * n]) for i in range(a.rounds)] if n else []
        if groups:
            med = statistics.median(groups)
            out[k] = {"dispatches": len(v), "round_means_us": [round(g, 2) for g in groups], "us": round(med, 2),
                      "us_min": round(min(groups), 2), "us_max": round(max(groups), 2),
                      "fastest_dispatch_us": round(min(v), 2), "GB_per_s": round(4 * a.snps / (med * 1e-6) / 1e9, 1)}
    if "k_div_win" in out and "k_fst_win" in out:
        out["div_over_fst"] = round(out["k_div_win"]["us"] / out["k_fst_win"]["us"], 3)
    print(json.dumps(out))
    sys.exit(0)

import torch  # noqa: E402
from sfs2d import _lib as L  # noqa: E402
from sfs2d.engine import Engine, ScanConfig  # noqa: E402
from sfs2d.synth import synth_genome  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("div_time: no GPU (timings are taken on the device only)")
p = synth_genome(1, a.snps, 25, 25, seed=777)
eng = Engine.get(0)
stream = torch.cuda.Stream()
eng.set_stream(stream.cuda_stream)
dev = eng.upload(p)
pl = eng.plan(dev, ScanConfig(n1p=25, n2p=25, window=20000, bg_mode=L.BG_PER_CHROM))
# k_fst_win on its own: a 20 kb Fst plan attached to a second, sliced 20 kb plan, its Fst not summed in the scan
# (SFS2D_FST_SCAN=0, read at plan creation): the base's run launches k_fst_win over the attached plan's slots
sl = eng.plan(dev, ScanConfig(n1p=25, n2p=25, window=20000, bg_mode=L.BG_PER_CHROM))
os.environ["SFS2D_FST_SCAN"] = "0"
at = sl.attach(ScanConfig(n1p=25, n2p=25, window=20000, fst=True, bg_mode=L.BG_PER_CHROM))
del os.environ["SFS2D_FST_SCAN"]
assert at.nrec == pl.nrec
buf = torch.empty(pl.nrec * L.DIVERSITY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
pl.run()
pl.check()
sl.run()          # warm-up of both kernels
sl.check()
pl.diversity(out_dev_ptr=buf.data_ptr())
stream.synchronize()
for _ in range(a.rounds):
    for _ in range(a.reps):
        sl.run()
        pl.diversity(out_dev_ptr=buf.data_ptr())
    stream.synchronize()
sl.check()


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


div_call = [event_ms(lambda: pl.diversity(out_dev_ptr=buf.data_ptr()), 50) * 1e3 for _ in range(a.rounds)]
passes = []
for _ in range(a.rounds):
    stream.synchronize()
    t0 = time.perf_counter()
    pl.run_many(200)
    stream.synchronize()
    passes.append((time.perf_counter() - t0) / 200 * 1e6)
pl.check()
recs = pl.read()
live = (recs["flags"] & (L.W_EMPTY | L.W_EXTRA)) == 0
print(json.dumps({"snps": p.n, "grid": [51, 51], "window": 20000, "records": int(pl.nrec), "windows": int(live.sum()),
                  "scan_kernel": pl.scan_kernel(), "rounds": a.rounds, "reps": a.reps,
                  "diversity_call_us": round(statistics.median(div_call), 2),
                  "diversity_call_us_min": round(min(div_call), 2), "diversity_call_us_max": round(max(div_call), 2),
                  "pass_us": round(statistics.median(passes), 2), "pass_us_min": round(min(passes), 2),
                  "pass_us_max": round(max(passes), 2)}))
sl.close()
pl.close()
dev.close()
