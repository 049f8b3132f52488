#!/usr/bin/env python3
"""Time a regions plan beside the sliding plan whose slots it is given.

DESIGN.md section 13's chromosome: one synthetic chromosome of 1e6 SNPs (synth_genome seed 12345, 25 + 25 diploids),
per-chromosome background, Fst on, k_scan_w.  Three plans on the same resident data, timed with Plan.time
(sfs2d_plan_time: the whole run, the stage before the tables = k_prep + the slot kernel, the tables, the scan):

  a  the sliding plan W = 20 kb, S = 5 kb;
  b  a regions plan given exactly those slots, (j S + 1, j S + W) (slot 0 from 0, as the sliding plan's) -- the same
     scan kernel over the same slot table, so (a) of the same session is its yardstick;
  c  a regions plan of 20,000 intervals with log-uniform lengths from 1 kb to 1 Mb at uniform places: gene-like and
     unbalanced (a record of what one 50,000-SNP region beside thousands of small ones does to a chunked scan).

The plans are run interleaved, `rounds` times `iters` iterations each; every figure is the median of the rounds, with
their minimum and maximum.  (b)'s table is compared with (a)'s before timing.  Prints one JSON line per plan.

usage: python tools/region_time.py [--rounds 5] [--iters 20] [--snps 1000000]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2dsfs-scan_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--snps", type=int, default=1_000_000)
ap.add_argument("--regions", type=int, default=20_000)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sfs2d import _lib as L  # noqa: E402
from sfs2d.engine import Engine, ScanConfig  # noqa: E402
from sfs2d.regions import Regions, region_ranges  # noqa: E402
from sfs2d.synth import synth_genome  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("region_time: no GPU (timings are taken on the device only)")
W, S = 20000, 5000
p = synth_genome(1, a.snps, 25, 25, seed=12345)
name, last = p.chrom_names[0], int(p.pos[-1])
tiles = Regions(p.chrom_names, [(name, j * S + 1 if j else 0, j * S + W) for j in range((last - 1) // S + 1)])
rng = np.random.Generator(np.random.PCG64(16))
length = np.exp(rng.uniform(np.log(1e3), np.log(1e6), size=a.regions)).astype(np.int64)
first = 1 + (rng.random(a.regions) * np.maximum(1, last - length)).astype(np.int64)
genes = Regions(p.chrom_names, [(name, int(f), int(f + n - 1), f"g{i}") for i, (f, n) in enumerate(zip(first, length))])

eng = Engine.get(0)
dev = eng.upload(p)
base = dict(n1p=25, n2p=25, bg_mode=L.BG_PER_CHROM, fst=True)
plans = {"a_sliding_20kb_5kb": eng.plan(dev, ScanConfig(window=W, step=S, **base)),
         "b_regions_same_slots": eng.plan(dev, ScanConfig(regions=tiles, **base)),
         "c_regions_gene_like": eng.plan(dev, ScanConfig(regions=genes, **base))}
for pl in plans.values():   # warm-up
    pl.run()
    pl.check()
ra, rb = plans["a_sliding_20kb_5kb"].read(), plans["b_regions_same_slots"].read()
assert ra.tobytes() == rb.tobytes(), "the regions plan's table is not the sliding plan's"
assert plans["a_sliding_20kb_5kb"].read_fst().tobytes() == plans["b_regions_same_slots"].read_fst().tobytes()
times = {k: [] for k in plans}
for _ in range(a.rounds):
    for k, pl in plans.items():
        times[k].append(pl.time(a.iters))
for k, pl in plans.items():
    rg = pl.cfg.regions
    out = {"plan": k, "snps": p.n, "slots": int(pl.nrec), "scan_kernel": pl.scan_kernel(), "seg": pl.seg_kind(),
           "variant": pl.scan_variant(), "rounds": a.rounds, "iters": a.iters}
    if rg is not None:
        b, e = region_ranges(p, rg)
        out["snps_per_region_max"] = int((e - b).max())
        out["snps_per_region_median"] = int(np.median(e - b))
        out["snps_scanned"] = int((e - b).sum())
    else:
        recs = pl.read()
        out["snps_scanned"] = int((recs["end"].astype(np.int64) - recs["begin"])[(recs["flags"] & L.W_EMPTY) == 0].sum())
    for i, what in enumerate(("run_ms", "slots_stage_ms", "tables_ms", "scan_ms")):
        v = [t[i] for t in times[k]]
        out[what] = round(statistics.median(v), 4)
        out[what + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    print(json.dumps(out))
for pl in plans.values():
    pl.close()
dev.close()
