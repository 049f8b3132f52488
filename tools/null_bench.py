#!/usr/bin/env python3
"""Time the bootstrap null (kernel k_null, sfs2d_plan_null_run) on a chromosome of config 3's size.

One synthetic chromosome of 1,562,500 SNPs (synth_genome, 25 + 25 diploids: n1 = n2 = 50), a fused
per-chromosome plan at 20 kb.  Kernel alone: one task (pool 0, m) with R = 10,000 replicates at m = 358
(the mean window), 16 and 4,096; each timed as `reps` calls between two events on the engine's stream after
a warm-up call (which also builds the plan's tables), median of `rounds` such timings; draws/s = m R / time.
Whole genome: the chromosome 32 times over as 32 pools (identical chromosomes: the timing does not depend on
their contents), the default size classes of the 20 kb scan's windows per pool, R = 999 -- one
Plan.null_run into a device buffer, host clock around the call and a stream synchronise -- beside the same
plan's scan pass (run + synchronise, median).  Prints one JSON line.

--block B[,B...] (block lengths, "window" = one run per replicate window) adds the block null (kernel
k_null_blk; block 1 is k_null) beside it: "kernel_blocks" -- the three single-task lines per block length,
the variants alternated inside every round, median of the rounds -- and "genome_blocks", the whole-genome
call at block 1 and at the last block length given, alternated.  Without it the output is unchanged.

usage: python tools/null_bench.py [--reps 50] [--rounds 5] [--pools 32] [--block 1,8,64,window]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2dsfs-scan_amd"))
import torch  # noqa: E402
from sfs2d import _lib as L  # noqa: E402
from sfs2d import null as N  # noqa: E402
from sfs2d.engine import Engine, ScanConfig  # noqa: E402
from sfs2d.pack import PackedSNPs  # noqa: E402
from sfs2d.synth import synth_genome  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--pools", type=int, default=32)
ap.add_argument("--snps", type=int, default=1_562_500)
ap.add_argument("--block", default=None, metavar="B[,B...]")
a = ap.parse_args()
blocks = []   # (name, block length)
for tok in (a.block.split(",") if a.block else []):
    blocks.append((tok, 0xFFFFFFFF if tok == "window" else int(tok)))
    if not 1 <= blocks[-1][1] <= 0xFFFFFFFF:
        sys.exit(f"null_bench: block length {tok!r} not in [1, 2^32) or 'window'")
if not torch.cuda.is_available():
    sys.exit("null_bench: no GPU (timings are taken on the device only)")

one = synth_genome(1, a.snps, 25, 25, seed=777)
eng = Engine.get(0)
stream = torch.cuda.Stream()
eng.set_stream(stream.cuda_stream)
cfg = ScanConfig(n1p=25, n2p=25, window=20000, bg_mode=L.BG_PER_CHROM)
out = {"snps_per_chrom": one.n, "grid": [51, 51]}


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


# ---- the kernel alone, one chromosome
dev = eng.upload(one)
pl = eng.plan(dev, cfg)
pl.run()
pl.check()
R = 10000
buf = torch.empty(R * 64, dtype=torch.uint8, device="cuda")
out["kernel"] = {}
for m in (358, 16, 4096):
    call = lambda: pl.null_run([(0, m)], R, 1, out_dev_ptr=buf.data_ptr())
    call()
    stream.synchronize()
    ms = [event_ms(call, a.reps) for _ in range(a.rounds)]
    med = statistics.median(ms)
    out["kernel"][str(m)] = {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                             "draws_per_s": m * R / (med * 1e-3), "replicates": R}
if blocks:   # the same lines per block length, alternated inside a round (block 1: k_null, the baseline)
    out["kernel_blocks"] = {}
    for m in (16, 358, 4096):
        calls = {nm: (lambda b=b: pl.null_run([(0, m)], R, 1, out_dev_ptr=buf.data_ptr(), block=b)) for nm, b in blocks}
        for c in calls.values():
            c()
        stream.synchronize()
        ms = {nm: [] for nm in calls}
        for _ in range(a.rounds):
            for nm, c in calls.items():
                ms[nm].append(event_ms(c, a.reps))
        out["kernel_blocks"][str(m)] = {
            nm: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                 "draws_per_s": m * R / (statistics.median(v) * 1e-3), "replicates": R} for nm, v in ms.items()}
pl.close()
dev.close()
del buf

# ---- a genome of `pools` such chromosomes: the scan pass and its whole null
k = a.pools
g = PackedSNPs(np.tile(one.counts, k), np.tile(one.pos, k), np.arange(k + 1, dtype=np.int64) * one.n,
               [f"chr{c:04d}" for c in range(k)], np.tile(one.ann_id, k), list(one.ann_names), one.pop1, one.pop2)
dev = eng.upload(g)
pl = eng.plan(dev, cfg)
pl.run()
pl.check()
recs = pl.read()
recs = recs[(recs["flags"] & (L.W_EMPTY | L.W_EXTRA)) == 0]
cls = N.size_classes(recs["end"].astype(np.int64) - recs["begin"].astype(np.int64))
tasks = sorted(set(zip(recs["chrom"].tolist(), cls.tolist())))
R = 999


def wall_ms(fn):
    stream.synchronize()
    t0 = time.perf_counter()
    fn()
    stream.synchronize()
    return (time.perf_counter() - t0) * 1e3


scan = [wall_ms(pl.run) for _ in range(a.rounds + 1)][1:]
buf = torch.empty(len(tasks) * R * 64, dtype=torch.uint8, device="cuda")
null_call = lambda: pl.null_run(tasks, R, 1, out_dev_ptr=buf.data_ptr())
null = [wall_ms(null_call) for _ in range(a.rounds + 1)][1:]
draws = R * sum(m for _, m in tasks)
out["genome"] = {"pools": k, "snps": g.n, "windows": int(len(recs)), "tasks": len(tasks), "replicates": R,
                 "classes_per_pool": len(tasks) / k, "class_min": int(min(m for _, m in tasks)),
                 "class_max": int(max(m for _, m in tasks)), "draws": draws,
                 "null_ms": round(statistics.median(null), 3), "null_ms_min": round(min(null), 3), "null_ms_max": round(max(null), 3),
                 "scan_pass_ms": round(statistics.median(scan), 3), "scan_pass_ms_min": round(min(scan), 3),
                 "scan_pass_ms_max": round(max(scan), 3),
                 "null_over_scan": statistics.median(null) / statistics.median(scan),
                 "draws_per_s": draws / (statistics.median(null) * 1e-3)}
if blocks:   # the whole-genome call, single SNPs and the last block length given, alternated
    pair = [("1", 1), blocks[-1]]
    calls = {nm: (lambda b=b: pl.null_run(tasks, R, 1, out_dev_ptr=buf.data_ptr(), block=b)) for nm, b in pair}
    ms = {nm: [wall_ms(c)][:0] for nm, c in calls.items()}   # (one untimed call each)
    for _ in range(a.rounds):
        for nm, c in calls.items():
            ms[nm].append(wall_ms(c))
    out["genome_blocks"] = {nm: {"null_ms": round(statistics.median(v), 3), "null_ms_min": round(min(v), 3),
                                 "null_ms_max": round(max(v), 3), "draws_per_s": draws / (statistics.median(v) * 1e-3)}
                            for nm, v in ms.items()}
pl.close()
dev.close()
print(json.dumps(out))
