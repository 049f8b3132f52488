"""Command line: VCF + popmap in, per-window statistics CSV out.

The reference's entry point is the notebook-style script at the bottom of
scripts/src/twoDSFS_class.py (1788-2040): load the SNP dict, run ``combined_scan`` at 20 kb and
500 kb and ``scan_perChr_bySNPs`` at 500 / 300 SNPs, and write each result with
``save_csv_stats`` (1884-1907; chromosome accessions renamed through chromosomes.txt, 1788-1797).
This CLI runs the same drivers on the GPU path, from the native VCF parser straight to the packed
arrays (no dict), every window size from one resident upload and one k_prep pass (multi_scan):

    python -m sfs2d VCF POPMAP --window 20000 --window 500000 --snp-window 500 \\
        --chromosomes chromosomes.txt --out-prefix ECBstats [--fst | --pixy-fst fst_20kb.csv]

Outputs ``<prefix>_20kb.csv``, ``<prefix>_500kb.csv``, ``<prefix>_500snps.csv`` with the reference's
columns; ``--fst`` appends an ``FST`` column with this framework's Hudson estimator,
``--pixy-fst FILE`` instead joins pixy's ``avg_wc_fst`` by (chromosome, window_start,
window_end) the way ECBstats_plots.R:16-41 does (pixy chromosome ``NC_087088_1`` -> ``NC_087088.1``)
-- the FST column of the published data/ECBstats_*.csv.

``--step BP`` makes every ``--window`` a sliding scan (windows advanced by BP, a divisor of each window;
multi_sliding_scan): ``<prefix>_20kb_step5kb.csv`` with the same columns, clean None rules.

``--null-replicates R [--null-seed S] [--null-sizes exact]`` appends six bootstrap p-value columns
(``p_T2D`` ... ``p_T2D_diff``, after ``FST`` when present) to every output file: R windows of the same
SNP count drawn from the window's chromosome per size class (scan_pvalues).
``--diversity`` appends twelve columns (``pi_pop1`` ... ``tajima_d_pop2``: per-site pi, dxy, da and Watterson's
theta, segregating sites, Tajima's D; sfs2d.diversity) after ``FST`` when present and before
the ``p_*`` columns, summed on the GPU over the data the scan already holds.
``--null-block B|window`` (with ``--null-replicates``) draws runs of B consecutive SNPs instead of single
SNPs, so that the null keeps the chromosome's linkage; ``window``: one run as long as the window.

``--regions FILE.bed`` scans the intervals of a BED file (genes, an inversion, candidate regions) as windows of
their own, from the same pass as the ``--window`` scans when there are any (a regions plan attached to them), and
writes ``<prefix>_regions.csv``: a leading ``name`` column (BED column 4, else ``<chrom> <first>-<last>``), then the
usual columns in the usual order, ``window_start`` / ``window_end`` the region's 1-based inclusive bounds; one row
per BED line in the file's order, a region without SNPs with ``snp_count`` 0 and empty fields.  ``--fst``,
``--diversity`` and ``--null-*`` apply to it; ``--regions`` alone scans nothing else.

``--outlier-spectra KEY:Q`` (repeatable; KEY one of T2D, T1D_p1, T1D_p2, new_term_p1, new_term_p2, T2D_diff, or FST
with ``--fst``; 0 < Q < 1) writes, for every ``--window`` / ``--snp-window`` / sliding output, the joint spectrum of
the windows whose KEY is at or above its Q quantile, pooled on the GPU (outlier_spectra):
``<prefix>_<size>_<KEY>_top<pct>.fs`` and ``..._background.fs`` (dadi's format; the background is the sum of the
whole-chromosome spectra of the chromosomes holding a selected window) and ``..._residuals.csv`` (``x1, x2,
fg_count, bg_count, fg_p, bg_p, diff, t2d_term`` for the bins where either count is non-zero).  The windows are
chosen from the statistics with the clean None rules of the sliding scans.  ``--region-spectra`` (with
``--regions``) writes ``<prefix>_regions_spectra.npz``: ``name``, ``sfs2d[nregions, n1 + 1, n2 + 1]``,
``sfs1d_pop1``, ``sfs1d_pop2`` in the BED file's order -- a spectrum per gene to hand to dadi / moments /
fastsimcoal.

``--project M1,M2`` (with ``--outlier-spectra`` or ``--region-spectra``; 2 <= M_k <= 2 pop_size_k) projects those
spectra down hypergeometrically to M1 / M2 haploid samples on the GPU, as dadi's
``projections=`` and easySFS do: only SNPs called in at least M_k alleles of both populations count, each spread
over the bins its subsamples fall in.  The file stems gain ``_proj<M1>x<M2>``, the grids are floats of
``(M1 + 1) x (M2 + 1)`` bins (foreground and background alike, folded unless ``--no-fold``; a tie of the joint fold
stays where it is, dadi averages ties), the npz gains ``n_used`` and ``n_dropped`` and its 1D spectra are the grid's
marginals; each output prints the share of its SNPs that the projection dropped.

``--project-scan M1,M2`` scans every window again at the common sample size M1 / M2 (projected_scan; DESIGN.md
section 19): T2D and T1D from the window's projected spectrum against its chromosome's, without the pull toward the
low bins that missing calls give a window.  One more file per ``--window`` / ``--snp-window`` / sliding /
``--regions`` output, ``<stem>_projscan<M1>x<M2>.csv``: ``chromosome, window_start, window_end`` (``name`` first for
regions), ``snp_count, n_used, n_dropped, T2D_proj, T1D_pop1_proj, T1D_pop2_proj, new_term_pop1_proj,
new_term_pop2_proj, T2D_diff_proj``; each prints the share of its SNPs that the projection dropped.  Every other
file is what it is without the flag.

``--project-null R`` (with ``--project-scan``; ``--null-seed`` is shared) appends to every such file the p-values of
the projected statistics from a null that keeps each window's called counts (projected_scan(replicates=R); DESIGN.md
section 20): ``p_T2D_proj, p_T1D_pop1_proj, p_T1D_pop2_proj, p_new_term_pop1_proj, p_new_term_pop2_proj,
p_T2D_diff_proj`` and ``n_thin``, the window's used SNPs whose stratum of equal called counts holds fewer than 8
SNPs; each file prints the share of used slots that are thin.  Without the flag every file is what it was.
"""
from __future__ import annotations

import argparse
import csv
import os
import re
import sys
import time


def _fmt_kb(ws: int) -> str:
    return f"{ws // 1000}kb" if ws % 1000 == 0 else f"{ws}bp"


def read_pixy_fst(path):
    """pixy windowed Fst CSV -> {(accession, start, end): avg_wc_fst} (ECBstats_plots.R:16-28)."""
    out = {}
    with open(path, newline="", encoding="utf-8-sig") as fh:
        for row in csv.DictReader(fh):
            chrom = re.sub(r"^(.*?_.*?)_(.*)$", r"\1.\2", row["chromosome"])
            v = row["avg_wc_fst"]
            out[(chrom, str(row["window_pos_1"]), str(row["window_pos_2"]))] = None if v in ("", "NA") else float(v)
    return out


P_COLS = ["p_T2D", "p_T1D_pop1", "p_T1D_pop2", "p_new_term_pop1", "p_new_term_pop2", "p_T2D_diff"]


def write_csv(path, stats, chr_ids, fst=None, pixy=None, pvalues=False, diversity=False):
    """save_csv_stats (twoDSFS_class.py:1884-1907) + optional FST column + optional diversity columns (the rows'
    sfs2d.diversity.KEYS, after FST) + optional p-value columns (the rows' p_* keys, scan_pvalues).  A None is
    an empty field, as for the statistics."""
    import twoDSFS_class as T
    from .diversity import KEYS as D_COLS
    cols = (list(T.col_names) + (["FST"] if (fst is not None or pixy is not None) else []) + (D_COLS if diversity else [])
            + (P_COLS if pvalues else []))
    with open(path, "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=cols)
        w.writeheader()
        for label, r in stats.items():
            chrom = label.split(" ")[0]
            s, e = label.split(" ")[1].split("-")
            row = {"chromosome": chr_ids.get(chrom, chrom), "window_start": s, "window_end": e,
                   "snp_count": r["snp_count"], "T2D": r["T2D"], "T1D_p1": r["T1D_pop1"], "T1D_p2": r["T1D_pop2"],
                   "new_term_p1": r["new_term_pop1"], "new_term_p2": r["new_term_pop2"],
                   "T2D_diff": r.get("T2D_diff")}
            if fst is not None:
                row["FST"] = fst.get(label)
            elif pixy is not None:
                row["FST"] = pixy.get((chrom, s, e))
            if diversity:
                for c in D_COLS:
                    row[c] = r.get(c)
            if pvalues:
                for c in P_COLS:
                    row[c] = r.get(c)
            w.writerow(row)


def write_regions_csv(path, rows, regions, chr_ids, fst=False, pvalues=False, diversity=False):
    """``<prefix>_regions.csv``: write_csv's columns behind a leading ``name`` column, one row per region of
    ``regions`` (a sfs2d.regions.Regions) in the caller's order; ``rows`` = the class's region rows."""
    import twoDSFS_class as T
    from .diversity import KEYS as D_COLS
    cols = (["name"] + list(T.col_names) + (["FST"] if fst else []) + (D_COLS if diversity else [])
            + (P_COLS if pvalues else []))
    with open(path, "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=cols)
        w.writeheader()
        for key, s in zip(regions.keys(), regions.slot.tolist()):
            r = rows[key]
            chrom = regions.chrom_names[int(regions.chrom[s])]
            row = {"name": key, "chromosome": chr_ids.get(chrom, chrom), "window_start": int(regions.first[s]),
                   "window_end": int(regions.last[s]), "snp_count": r["snp_count"], "T2D": r["T2D"],
                   "T1D_p1": r["T1D_pop1"], "T1D_p2": r["T1D_pop2"], "new_term_p1": r["new_term_pop1"],
                   "new_term_p2": r["new_term_pop2"], "T2D_diff": r.get("T2D_diff")}
            if fst:
                row["FST"] = r.get("FST")
            for c in (D_COLS if diversity else []) + (P_COLS if pvalues else []):
                row[c] = r.get(c)
            w.writerow(row)


# --outlier-spectra KEY: the CSV's statistic columns -> the rows' keys
SPECTRA_KEYS = {"T2D": "T2D", "T1D_p1": "T1D_pop1", "T1D_p2": "T1D_pop2", "new_term_p1": "new_term_pop1",
                "new_term_p2": "new_term_pop2", "T2D_diff": "T2D_diff", "FST": "FST"}


def parse_outlier_spec(text):
    """``KEY:Q`` -> (KEY, Q); ValueError with the reason for a malformed one."""
    key, sep, qs = str(text).partition(":")
    if not sep or key not in SPECTRA_KEYS:
        raise ValueError(f"--outlier-spectra {text!r}: expected KEY:Q with KEY one of {', '.join(SPECTRA_KEYS)}")
    try:
        q = float(qs)
    except ValueError:
        q = float("nan")
    if not 0.0 < q < 1.0:
        raise ValueError(f"--outlier-spectra {text!r}: Q must be a number in (0, 1)")
    return key, q


def parse_project(text, n1p: int, n2p: int, flag: str = "--project"):
    """``M1,M2`` -> (M1, M2); ValueError with the reason for a malformed or out-of-range one."""
    try:
        m1, m2 = (int(x) for x in str(text).split(","))
    except ValueError:
        raise ValueError(f"{flag} {text!r}: expected M1,M2 (two integers)") from None
    if not (2 <= m1 <= 2 * n1p and 2 <= m2 <= 2 * n2p):
        raise ValueError(f"{flag} {text!r}: need 2 <= M1 <= {2 * n1p} and 2 <= M2 <= {2 * n2p}")
    return m1, m2


def write_projscan_csv(path, rows, chr_ids, regions=None, null=False):
    """``<stem>_projscan<M1>x<M2>.csv``: the rows of projected_scan (sfs2d.spectra.PROJSCAN_COLUMNS) behind the
    window's chromosome, start and end, with a leading ``name`` column for ``regions`` (one row per region in the
    caller's order).  ``null``: the rows carry projected_scan(replicates=...)'s p-values and n_thin, appended as
    seven more columns.  A None is an empty field."""
    from .spectra import PROJSCAN_COLUMNS
    head = ["chromosome", "window_start", "window_end"]
    cols = list(PROJSCAN_COLUMNS)
    if null:   # (--project-null: the seven columns of sfs2d.projnull behind the others)
        from .projnull import PROJNULL_COLUMNS
        cols += PROJNULL_COLUMNS
    with open(path, "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=(["name"] if regions is not None else []) + head + cols)
        w.writeheader()
        if regions is not None:
            for key, s in zip(regions.keys(), regions.slot.tolist()):
                chrom = regions.chrom_names[int(regions.chrom[s])]
                w.writerow({"name": key, "chromosome": chr_ids.get(chrom, chrom), "window_start": int(regions.first[s]),
                            "window_end": int(regions.last[s]), **rows[key]})
            return
        for label, r in rows.items():
            chrom = label.split(" ")[0]
            s, e = label.split(" ")[1].split("-")
            w.writerow({"chromosome": chr_ids.get(chrom, chrom), "window_start": s, "window_end": e, **r})


def _dropped_share(used, dropped) -> str:
    n = int(used) + int(dropped)
    return f"{int(dropped)} of {n} SNPs dropped ({100.0 * int(dropped) / n:.2f} %)" if n else "no SNPs"


def _fmt_pct(q: float) -> str:
    return f"{round((1.0 - q) * 100.0, 6):g}"


def write_outlier_spectra(stem, res, folded, pop_ids):
    """The three files of one outlier_spectra result ``res`` under ``stem``; returns their paths."""
    from . import spectra as SP
    paths = [f"{stem}.fs", f"{stem}_background.fs", f"{stem}_residuals.csv"]
    SP.write_dadi_fs(paths[0], res["foreground"], folded, pop_ids)
    SP.write_dadi_fs(paths[1], res["background"], folded, pop_ids)
    with open(paths[2], "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(SP.RESIDUAL_COLUMNS)
        w.writerows(SP.residual_rows(res["residuals"]))
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m sfs2d", description=__doc__.split("\n\n")[0])
    ap.add_argument("vcf")
    ap.add_argument("popmap")
    ap.add_argument("--pop1", default="uv")
    ap.add_argument("--pop2", default="bv")
    ap.add_argument("--pop1-size", type=int, default=18, help="diploid individuals of pop1 (twoDSFS_class.py:22)")
    ap.add_argument("--pop2-size", type=int, default=14)
    ap.add_argument("--window", type=int, action="append", default=[], help="fixed-bp window (combined_scan)")
    ap.add_argument("--snp-window", type=int, action="append", default=[], help="SNPs per window (scan_perChr_bySNPs)")
    ap.add_argument("--step", type=int, default=None, metavar="BP",
                    help="sliding windows: advance every --window by BP (a divisor of it, >= window / 64)")
    ap.add_argument("--variant-type", default=None)
    ap.add_argument("--no-fold", action="store_true")
    ap.add_argument("--chromosomes", default=None, help="accession<TAB>number map (chromosomes.txt)")
    ap.add_argument("--fst", action="store_true", help="append Hudson's Fst (this framework's estimator)")
    ap.add_argument("--pixy-fst", default=None, help="join pixy avg_wc_fst as the FST column")
    ap.add_argument("--null-replicates", type=int, default=None, metavar="R",
                    help="append bootstrap p-values: R resampled windows per chromosome and size class")
    ap.add_argument("--null-seed", type=int, default=0, metavar="S")
    ap.add_argument("--null-sizes", choices=["exact"], default=None,
                    help="exact: a null for every distinct SNP count (default: a 9 %% geometric grid of sizes)")
    ap.add_argument("--null-block", default=None, metavar="B|window",
                    help="resample runs of B consecutive SNPs (window: one run per replicate window) instead of "
                         "single SNPs; needs --null-replicates")
    ap.add_argument("--diversity", action="store_true",
                    help="append per-window pi, dxy, da, Watterson's theta, S and Tajima's D (twelve columns)")
    ap.add_argument("--regions", default=None, metavar="FILE.bed",
                    help="scan the intervals of a BED file as windows of their own -> <prefix>_regions.csv")
    ap.add_argument("--outlier-spectra", action="append", default=[], metavar="KEY:Q",
                    help="pooled joint SFS of the windows with KEY at or above its Q quantile, its background and "
                         "their per-bin residuals -> <prefix>_<size>_<KEY>_top<pct>{.fs,_background.fs,_residuals.csv}")
    ap.add_argument("--region-spectra", action="store_true",
                    help="with --regions: every region's 2D and folded 1D spectra -> <prefix>_regions_spectra.npz")
    ap.add_argument("--project", default=None, metavar="M1,M2",
                    help="with --outlier-spectra / --region-spectra: project the spectra down to M1 / M2 haploid "
                         "samples (SNPs with fewer called alleles are dropped); stems gain _proj<M1>x<M2>")
    ap.add_argument("--project-scan", default=None, metavar="M1,M2",
                    help="T2D / T1D of every window at the common sample size M1 / M2 (projected spectra against the "
                         "projected chromosome) -> one <stem>_projscan<M1>x<M2>.csv per window output")
    ap.add_argument("--project-null", type=int, default=None, metavar="R",
                    help="with --project-scan: append p-values from R replicates per window whose SNPs are redrawn "
                         "among SNPs of equal called counts (seven columns; --null-seed is the draws' seed)")
    ap.add_argument("--out-prefix", default="stats")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--threads", type=int, default=0, help="VCF parser threads (0 = all)")
    a = ap.parse_args(argv)
    if not a.window and not a.snp_window and a.regions is None:
        a.window = [20000]
    if a.null_replicates is not None and a.null_replicates < 1:
        ap.error("--null-replicates must be >= 1")
    ospecs = []
    for text in a.outlier_spectra:
        try:
            ospecs.append(parse_outlier_spec(text))
        except ValueError as e:
            ap.error(str(e))
        if ospecs[-1][0] == "FST" and not a.fst:
            ap.error("--outlier-spectra FST:Q needs --fst")
    if a.region_spectra and a.regions is None:
        ap.error("--region-spectra needs --regions")
    pkw, ptag = {}, ""   # (without the flag every call below is the one it was)
    if a.project is not None:
        if not ospecs and not a.region_spectra:
            ap.error("--project applies to --outlier-spectra / --region-spectra: give one of them")
        try:
            pkw = dict(project=parse_project(a.project, a.pop1_size, a.pop2_size))
        except ValueError as e:
            ap.error(str(e))
        ptag = "_proj{}x{}".format(*pkw["project"])
    pscan = None
    if a.project_scan is not None:
        try:
            pscan = parse_project(a.project_scan, a.pop1_size, a.pop2_size, "--project-scan")
        except ValueError as e:
            ap.error(str(e))
    if a.project_null is not None:
        if pscan is None:
            ap.error("--project-null needs --project-scan")
        if a.project_null < 1:
            ap.error("--project-null must be >= 1")
    pnkw = dict(replicates=a.project_null, seed=a.null_seed) if a.project_null is not None else {}
    null = a.null_replicates is not None
    block = None
    if a.null_block is not None:
        if not null:
            ap.error("--null-block needs --null-replicates")
        if a.null_block == "window":
            block = "window"
        else:
            try:
                block = int(a.null_block)
            except ValueError:
                block = 0
            if not 1 <= block < (1 << 32):
                ap.error("--null-block must be an integer in [1, 2^32) or 'window'")
    nkw = dict(replicates=a.null_replicates, seed=a.null_seed, sizes=a.null_sizes, block=block)
    dkw = dict(diversity=True) if a.diversity else {}   # (without the flag every call is the one it was)
    if a.step is not None:
        if a.snp_window:
            ap.error("--step applies to fixed-bp windows: not with --snp-window")
        if a.step < 1:
            ap.error("--step must be >= 1")
        for ws in a.window:
            if ws < a.step or ws % a.step != 0:
                ap.error(f"--step {a.step} does not divide --window {ws}")
            if ws // a.step > 64:
                ap.error(f"--window {ws} is more than 64 steps of {a.step}")

    import twoDSFS_class as T
    from sfs2d.vcf import make_packed_vcf

    t0 = time.perf_counter()
    packed = make_packed_vcf(a.vcf, a.popmap, a.pop1, a.pop2, nthreads=a.threads)
    t1 = time.perf_counter()
    print(f"ingest: {packed.n} SNPs, {packed.nchrom} chromosomes in {t1 - t0:.3f} s", file=sys.stderr)
    chr_ids = T.load_chr_ids(a.chromosomes) if a.chromosomes else {}
    pixy = read_pixy_fst(a.pixy_fst) if a.pixy_fst else None
    obj = T.LikelihoodInference_jointSFS(a.vcf, a.popmap, pop1=a.pop1, pop2=a.pop2, pop1_size=a.pop1_size,
                                         pop2_size=a.pop2_size, variant_type=a.variant_type, fold=not a.no_fold,
                                         device=a.device)
    outs = []
    rg, rkw = None, {}
    if a.regions is not None:   # (without the flag every call below is the one it was)
        from .regions import Regions
        rg = Regions.from_bed(packed, a.regions)
        rkw = dict(regions=rg)

    def projscan_out(stem, **geometry):
        # (the new flag alone: a scan of its own per file, nothing of the calls above changes)
        if pscan is None:
            return
        rows = obj.projected_scan(packed, pscan, **geometry, **pnkw)
        path = "{}_projscan{}x{}.csv".format(stem, *pscan)
        write_projscan_csv(path, rows, chr_ids, geometry.get("regions"), **(dict(null=True) if pnkw else {}))
        outs.append(path)
        used, dropped = (sum(r[k] for r in rows.values()) for k in ("n_used", "n_dropped"))
        print(f"projected_scan {pscan}: {len(rows)} windows, {_dropped_share(used, dropped)} -> {path}", file=sys.stderr)
        if pnkw:
            thin = sum(r["n_thin"] for r in rows.values())
            share = f"{100.0 * thin / used:.2f} %" if used else "no used SNPs"
            print(f"project_null R = {a.project_null}: {thin} of {used} used slots are thin ({share}: strata of fewer "
                  f"than 8 SNPs)", file=sys.stderr)

    def regions_out(res):
        if rg is None:
            return
        path = f"{a.out_prefix}_regions.csv"
        write_regions_csv(path, res["regions"], rg, chr_ids, a.fst, null, a.diversity)
        outs.append(path)
        print(f"region_scan: {len(rg)} regions -> {path}", file=sys.stderr)
        projscan_out(f"{a.out_prefix}_regions", regions=rg)

    def spectra_out(size, **geometry):
        # (the new flags alone: a scan of its own per file, nothing of the calls above changes)
        for key, q in ospecs:
            res = obj.outlier_spectra(packed, key=SPECTRA_KEYS[key], q=q, fst=key == "FST", **geometry, **pkw)
            stem = f"{a.out_prefix}_{size}_{key}_top{_fmt_pct(q)}{ptag}"
            outs.extend(write_outlier_spectra(stem, res, not a.no_fold, (a.pop1, a.pop2)))
            print(f"outlier_spectra {size} {key} >= q{q:g}: {len(res['labels'])} windows, pooled T2D {res['T2D']} -> "
                  f"{stem}.fs", file=sys.stderr)
            if pkw:
                print(f"projection {pkw['project']}: foreground {_dropped_share(res['n_used'], res['n_dropped'])}, "
                      f"background {_dropped_share(res['background_n_used'], res['background_n_dropped'])}", file=sys.stderr)

    def region_spectra_out():
        if not a.region_spectra:
            return
        import numpy as np
        sp = obj.window_spectra(packed, regions=rg, **pkw)
        keys = rg.keys()
        path = f"{a.out_prefix}_regions_spectra{ptag}.npz"
        extra = {k: np.array([sp[r][k] for r in keys], np.int64) for k in (("n_used", "n_dropped") if pkw else ())}
        np.savez(path, name=np.array(keys, dtype=str), sfs2d=np.stack([sp[k]["sfs2d"] for k in keys]),
                 sfs1d_pop1=np.stack([sp[k]["sfs1d_pop1"] for k in keys]),
                 sfs1d_pop2=np.stack([sp[k]["sfs1d_pop2"] for k in keys]), **extra)
        outs.append(path)
        print(f"window_spectra: {len(keys)} regions -> {path}", file=sys.stderr)
        if pkw:
            print(f"projection {pkw['project']}: {_dropped_share(extra['n_used'].sum(), extra['n_dropped'].sum())}",
                  file=sys.stderr)
    t = time.perf_counter()
    if a.step is not None:   # sliding windows: every size from one upload and one k_prep pass
        if null:
            res = obj.scan_pvalues(packed, a.window, step_size=a.step, fst=a.fst, **nkw, **dkw, **rkw)
        else:
            res = obj.multi_sliding_scan(packed, a.window, a.step, fst=a.fst, **dkw, **rkw)
        print(f"multi_sliding_scan ({len(a.window)} window sizes, step {a.step}): {time.perf_counter() - t:.2f} s",
              file=sys.stderr)
        for ws in a.window:
            path = f"{a.out_prefix}_{_fmt_kb(ws)}_step{_fmt_kb(a.step)}.csv"
            rows = res[ws]
            write_csv(path, rows, chr_ids, {k: r["FST"] for k, r in rows.items()} if a.fst else None, pixy, null, **dkw)
            outs.append(path)
            print(f"sliding_scan {ws} bp / {a.step} bp: {len(rows)} windows -> {path}", file=sys.stderr)
            spectra_out(f"{_fmt_kb(ws)}_step{_fmt_kb(a.step)}", window_size=ws, step_size=a.step)
            projscan_out(path[:-4], window_size=ws, step_size=a.step)
        regions_out(res)
        region_spectra_out()
        return outs
    # every window size from one k_prep pass over the resident stream (sfs2d_plan_attach)
    if null:
        res = obj.scan_pvalues(packed, a.window, a.snp_window, fst=a.fst, **nkw, **dkw, **rkw)
    else:
        res = obj.multi_scan(packed, a.window, a.snp_window, fst=a.fst, **dkw, **rkw)
    print(f"multi_scan ({len(a.window)} bp + {len(a.snp_window)} SNP-count window sizes): "
          f"{time.perf_counter() - t:.2f} s", file=sys.stderr)
    for ws in a.window:
        path = f"{a.out_prefix}_{_fmt_kb(ws)}.csv"
        write_csv(path, res[ws], chr_ids, res["fst"][ws] if a.fst else None, pixy, null, **dkw)
        outs.append(path)
        print(f"combined_scan {ws} bp: {len(res[ws])} windows -> {path}", file=sys.stderr)
        spectra_out(_fmt_kb(ws), window_size=ws)
        projscan_out(path[:-4], window_size=ws)
    for S in a.snp_window:
        stats = res[f"{S}snps"]
        fst = obj.window_fst(packed, snp_window_size=S) if a.fst else None
        path = f"{a.out_prefix}_{S}snps.csv"
        write_csv(path, stats, chr_ids, fst, pixy, null, **dkw)
        outs.append(path)
        print(f"scan_perChr_bySNPs {S} SNPs: {len(stats)} windows -> {path}", file=sys.stderr)
        spectra_out(f"{S}snps", snp_window_size=S)
        projscan_out(path[:-4], snp_window_size=S)
    regions_out(res)
    region_spectra_out()
    return outs


if __name__ == "__main__":
    main()
