"""Drop-in replacement for the reference module ``scripts/src/twoDSFS_class.py``.

Same class, method names, arguments, return shapes and error behaviour as the reference's
``LikelihoodInference_jointSFS`` (twoDSFS_class.py:20-1737) for the window-scan path, plus the
module-level ``col_names`` / ``chr_ids`` / ``save_csv_stats`` CSV writer (1788-1797, 1881-1907).
Every window statistic is computed by the HIP kernels of ``csrc/sfs2d.hip`` on an MI355X
(through ``sfs2d.engine``); there is no CPU fallback.

Methods accept either the reference's SNP dict (``{"CHR-POS": {"calls": ..., "annotation": ...}}``)
or an already packed ``sfs2d.PackedSNPs`` (skips the dict packing, which dominates host time).
"""
from __future__ import annotations

import csv
import os
from typing import Optional

import numpy as np

from sfs2d import _lib as L
from sfs2d import post
from sfs2d.engine import Engine, ScanConfig
from sfs2d.vcf import make_data_dict_vcf as _make_data_dict_vcf
from sfs2d.pack import PackedSNPs, last_key_index, pack_snp_dict, shadow_chrom_starts

__all__ = ["LikelihoodInference_jointSFS", "save_csv_stats", "col_names", "chr_ids", "load_chr_ids"]

_NO_ANN = 1 << 20   # an annotation id no SNP carries (variant_type absent from the data)

col_names = ['chromosome', 'window_start', 'window_end', 'snp_count', 'T2D', 'T1D_p1', 'T1D_p2',
             'new_term_p1', 'new_term_p2', 'T2D_diff']
chr_ids: dict = {}


def load_chr_ids(path: str) -> dict:
    """Accession -> chromosome number map (chromosomes.txt; reference 1788-1797)."""
    chr_ids.clear()
    with open(path, "r") as fh:
        for line in fh:
            columns = line.strip().split("\t")
            if len(columns) >= 2:
                chr_ids[columns[0]] = columns[1]
    return chr_ids


if os.environ.get("SFS2D_CHROMOSOMES"):
    load_chr_ids(os.environ["SFS2D_CHROMOSOMES"])


def save_csv_stats(stats_dict, output):
    """twoDSFS_class.py:1884-1907: one row per window, chromosome renamed through chr_ids."""
    with open(output, 'w', newline='') as csvfile:
        writer = csv.DictWriter(csvfile, fieldnames=col_names)
        writer.writeheader()
        for window_coords, result in stats_dict.items():
            chromosome = window_coords.split(' ')[0]
            chromosome_num = chr_ids.get(chromosome, chromosome)
            window_start, window_end = window_coords.split(' ')[1].split('-')
            writer.writerow({
                'chromosome': chromosome_num, 'window_start': window_start, 'window_end': window_end,
                'snp_count': result["snp_count"], 'T2D': result["T2D"], 'T1D_p1': result["T1D_pop1"],
                'T1D_p2': result["T1D_pop2"], 'new_term_p1': result["new_term_pop1"],
                'new_term_p2': result["new_term_pop2"], 'T2D_diff': result["T2D_diff"]})


def _fold_counts(u: np.ndarray) -> np.ndarray:
    """fold_1d_sfs on a dense unfolded spectrum: folded[f] = u[f] + u[2n-f], folded[n] = u[n]."""
    n2 = len(u) - 1
    n = n2 // 2
    out = np.zeros(n + 1, dtype=u.dtype)
    for f in range(n2 + 1):
        out[min(f, n2 - f)] += u[f]
    return out


class LikelihoodInference_jointSFS:
    def __init__(self, vcf_filename, popinfo_filename, start_position=None, end_position=None,
                 pop1='uv', pop2='bv', pop1_size=18, pop2_size=14, variant_type=None, fold=True, device=0,
                 distributed=False):
        """The reference's constructor (twoDSFS_class.py:21-33), plus ``device`` (the GPU of this
        process) and ``distributed``: with a torch.distributed process group (one process per GPU),
        every window scan is split over the group at window boundaries balanced by SNPs -- one
        chromosome spread over several ranks, its background histograms all-reduced -- and every rank
        returns the whole result (sfs2d.dist.scan_records_split); ``distributed="chromosomes"`` shards
        whole chromosomes instead (no collective before the scan; sfs2d.dist.scan_records).  All
        ranks must make the same calls."""
        self.vcf_filename = vcf_filename
        self.popinfo_filename = popinfo_filename
        self.pop1 = pop1
        self.pop2 = pop2
        self.pop1_size = pop1_size
        self.pop2_size = pop2_size
        self.start_position = start_position
        self.end_position = end_position
        self.variant_type = variant_type
        self.fold = fold
        self.device = device
        self.distributed = distributed

    # ------------------------------------------------------------------ ingest
    def make_data_dict_vcf(self, vcf_filename=None, popinfo_filename=None):
        """twoDSFS_class.py:36-138 (quirks Q12/Q13 kept; see sfs2d.vcf)."""
        return _make_data_dict_vcf(vcf_filename if vcf_filename is not None else self.vcf_filename,
                                   popinfo_filename if popinfo_filename is not None else self.popinfo_filename)

    # ------------------------------------------------------------------ plumbing
    def _engine(self) -> Engine:
        return Engine.get(self.device)

    def _pack(self, data, pop1=None, pop2=None) -> PackedSNPs:
        if isinstance(data, PackedSNPs):
            return data
        return pack_snp_dict(data, pop1 or self.pop1, pop2 or self.pop2)

    def _cfg(self, p: PackedSNPs, **kw) -> ScanConfig:
        ann = -1
        if self.variant_type is not None:
            ann = p.ann_names.index(self.variant_type) if self.variant_type in p.ann_names else _NO_ANN
        start = None if self.start_position is None else int(self.start_position)
        end = None if self.end_position is None else int(self.end_position)
        return ScanConfig(n1p=self.pop1_size, n2p=self.pop2_size, fold=bool(self.fold), ann_want=ann,
                          start_position=start, end_position=end, **kw)

    def _scan(self, p: PackedSNPs, cfg: ScanConfig, bg=None):
        if self.distributed:
            from sfs2d import dist as D
            if self.distributed == "chromosomes":
                return D.scan_records(p, cfg, bg, self._scan_local, self.device)
            return D.scan_records_split(p, cfg, bg, self._split_scan, self.device)
        return self._scan_local(p, cfg, bg)

    def _split_scan(self, p: PackedSNPs, cfg: ScanConfig, bg=None):
        from sfs2d.engine import SplitJob
        return SplitJob(self._engine(), p, cfg, bg)
    _split_scan.device_rows = True   # its jobs exchange background rows in HBM (sfs2d.dist._split_device)

    def _hist(self, p: PackedSNPs, cfg: ScanConfig, chrom: int):
        """Background histograms (h2d, unfolded h1a, unfolded h1b) of chromosome ``chrom`` (-1: all
        SNPs) on the GPU; distributed: every rank histograms a slice, one all-reduce on the device
        (sfs2d.dist.sharded_bg_hist)."""
        if self.distributed:
            from sfs2d import dist as D
            return D.sharded_bg_hist(p, cfg, self.device, chrom)
        eng = self._engine()
        dev = eng.upload(p if chrom < 0 else p.subset_chroms([chrom]))
        try:
            return eng.bg_hist(dev, cfg, -1)
        finally:
            dev.close()

    def _scan_local(self, p: PackedSNPs, cfg: ScanConfig, bg=None):
        eng = self._engine()
        dev = eng.upload(p)
        try:
            recs = eng.scan(dev, cfg, bg)
        finally:
            dev.close()
        return recs

    def _bg_arrays(self, p: PackedSNPs, chrom: int):
        """Unnormalised background of one chromosome (2D grid + folded 1D), computed on the GPU
        (distributed: sharded over the ranks, one all-reduce)."""
        h2, u1, u2 = self._hist(p, self._cfg(p), chrom)
        return h2, _fold_counts(u1), _fold_counts(u2)

    # ------------------------------------------------------------------ window scans
    def combined_scan(self, data_dict, window_size):
        """Each chromosome is its own background (twoDSFS_class.py:787-991)."""
        self.data_dict = data_dict
        self.window_size = window_size
        p = self._pack(data_dict)
        recs = self._scan(p, self._cfg(p, window_mode=L.WINDOW_BP, window=window_size,
                                       bg_mode=L.BG_PER_CHROM, prev_extra=True))
        return post.combined_scan(recs, p, window_size, post.num_slots(recs))

    def scan_chooseChr(self, data_dict, window_size, background_chromosome):
        """One named chromosome as the background for every window (993-1159)."""
        self.data_dict = data_dict
        self.window_size = window_size
        p = self._pack(data_dict)
        if background_chromosome not in p.chrom_names:
            raise ValueError(f"Background chromosome {background_chromosome} not found in the data.")
        bg = self._bg_arrays(p, p.chrom_names.index(background_chromosome))
        recs = self._scan(p, self._cfg(p, window_mode=L.WINDOW_BP, window=window_size,
                                       bg_mode=L.BG_SUPPLIED), bg)
        return post.fixed_bg_scan(recs, p, window_size, post.num_slots(recs))

    def scan_precomputed_BG(self, data_dict, window_size, bg_2d_sfs, bg_1d_sfs_pop1, bg_1d_sfs_pop2):
        """Caller-supplied (normalised or not) background SFS dicts (1161-1299)."""
        self.data_dict = data_dict
        self.window_size = window_size
        p = self._pack(data_dict)
        bg = (self._bg2d_array(bg_2d_sfs), self._bg1d_array(bg_1d_sfs_pop1, self.pop1_size),
              self._bg1d_array(bg_1d_sfs_pop2, self.pop2_size))
        recs = self._scan(p, self._cfg(p, window_mode=L.WINDOW_BP, window=window_size,
                                       bg_mode=L.BG_SUPPLIED), bg)
        return post.fixed_bg_scan(recs, p, window_size, post.num_slots(recs))

    def scan_chooseChr_bySNPs(self, data_dict, snp_window_size, background_chromosome):
        """Fixed-SNP windows against one named chromosome's NORMALISED background (1303-1420)."""
        self.data_dict = data_dict
        self.snp_window_size = snp_window_size
        p = self._pack(data_dict)
        if background_chromosome not in p.chrom_names:
            raise ValueError(f"Background chromosome {background_chromosome} not found in the data.")
        h2, f1, f2 = self._bg_arrays(p, p.chrom_names.index(background_chromosome))
        bg = (np.array(self._normalize_values(h2.ravel().tolist())),
              np.array(self._normalize_values(f1.tolist())), np.array(self._normalize_values(f2.tolist())))
        recs = self._scan(p, self._cfg(p, window_mode=L.WINDOW_SNPS, window=snp_window_size,
                                       bg_mode=L.BG_SUPPLIED), bg)
        return post.bysnp_scan(recs, p, snp_window_size, with_diff=False, final_warning=True)

    def scan_perChr_bySNPs(self, data_dict, snp_window_size):
        """Fixed-SNP windows, each chromosome its own background (1422-1541)."""
        self.data_dict = data_dict
        self.num_snps = snp_window_size
        p = self._pack(data_dict)
        recs = self._scan(p, self._cfg(p, window_mode=L.WINDOW_SNPS, window=snp_window_size,
                                       bg_mode=L.BG_PER_CHROM))
        return post.bysnp_scan(recs, p, snp_window_size, with_diff=True, final_warning=False)

    # ------------------------------------------------------------------ single-statistic scans
    def _filters(self, p: PackedSNPs):
        ann = -1
        if self.variant_type is not None:
            ann = p.ann_names.index(self.variant_type) if self.variant_type in p.ann_names else _NO_ANN
        return ann

    def T1D_scan(self, data_dict, background_sfs, window_size, pop, pop_size):
        """T1D of population ``pop`` (``pop_size`` individuals) per fixed-bp window against a supplied
        folded 1D background (twoDSFS_class.py:539-623): raw alt counts of ``pop`` (no joint fold),
        folded against 2*pop_size (:576-578), the constructor's position / variant_type filters.
        Returns {label: {"snp_count", "T1D"}}; T1D None for an empty window or background."""
        self.data_dict = data_dict
        self.background_sfs = background_sfs
        self.window_size = window_size
        self.pop = pop
        self.pop_size = pop_size
        p = self._pack(data_dict, pop1=pop, pop2=pop).single_pop(pop)
        if p.n == 0:
            return {}
        n = 2 * int(pop_size)
        # pop in both count slots, no fold: the 2D key (alt, alt) is in the grid exactly when the 1D
        # key is; the 2D statistic (against a dummy background) is not read
        cfg = ScanConfig(n1p=pop_size, n2p=pop_size, fold=False, ann_want=self._filters(p),
                         start_position=None if self.start_position is None else int(self.start_position),
                         end_position=None if self.end_position is None else int(self.end_position),
                         window_mode=L.WINDOW_BP, window=window_size, bg_mode=L.BG_SUPPLIED)
        bg = (np.ones((n + 1) * (n + 1)), self._bg1d_array(background_sfs, pop_size), np.ones(pop_size + 1))
        recs = self._scan(p, cfg, bg)
        return post.single_stat_scan(recs, p, window_size, post.num_slots(recs), 1, "T1D")

    def T2D_scan(self, data_dict, background_2d_sfs, window_size):
        """T2D per fixed-bp window against the SUPPLIED background (twoDSFS_class.py:686-776).  The
        per-chromosome background the reference computes at each chromosome change (:738-744) is not
        used for scoring (:753, :768 read ``self.background_2d_sfs``), but its loop rebinds the SNP key:
        the stream is rebuilt accordingly (``sfs2d.pack.shadow_chrom_starts``).
        Returns {label: {"snp_count", "T2D"}}; T2D None for an empty window or background."""
        self.data_dict = data_dict
        self.background_2d_sfs = background_2d_sfs
        self.window_size = window_size
        p = self._pack(data_dict)
        if p.n == 0:
            return {}
        q = shadow_chrom_starts(p, last_key_index(data_dict, p), window_size, self.start_position, self.end_position)
        cfg = ScanConfig(n1p=self.pop1_size, n2p=self.pop2_size, fold=bool(self.fold), ann_want=self._filters(q),
                         window_mode=L.WINDOW_BP, window=window_size, bg_mode=L.BG_SUPPLIED)
        bg = (self._bg2d_array(background_2d_sfs), np.ones(self.pop1_size + 1), np.ones(self.pop2_size + 1))
        recs = self._scan(q, cfg, bg)
        return post.single_stat_scan(recs, q, window_size, post.num_slots(recs), 2, "T2D")

    # ------------------------------------------------------------------ multi-resolution (extension)
    def multi_scan(self, data_dict, window_sizes=(), snp_window_sizes=(), fst=False, diversity=False, regions=None):
        """combined_scan at every size in ``window_sizes`` and scan_perChr_bySNPs at every size in
        ``snp_window_sizes`` from ONE pass over the SNP stream (the reference script runs these
        scans one after another over the same data, twoDSFS_class.py:1923-2032): the smallest
        fixed-bp scan is the base plan, the others are attached to it (sfs2d_plan_attach).
        Returns {ws: combined_scan result, "<S>snps": scan_perChr_bySNPs result}, plus
        {"fst": {ws: window_fst result}} when ``fst`` (fixed-bp windows only).  ``diversity``: every row
        also holds the twelve columns of ``window_diversity`` (sfs2d.diversity.KEYS), summed on the GPU over
        the same resident data (k_div_win after the run).  ``regions`` (as in ``region_scan``): the per-region rows
        as well, under the "regions" key, from a regions plan attached to the same base -- the tiled scan and the
        per-gene rows from one pass."""
        if regions is None:
            return self._multi_scan(data_dict, window_sizes, snp_window_sizes, fst, diversity=diversity)
        return self._multi_scan(data_dict, window_sizes, snp_window_sizes, fst, diversity=diversity, regions=regions)

    def _no_distributed_diversity(self, diversity):
        if diversity and self.distributed:
            raise NotImplementedError("diversity is single-GPU (distributed sharding of the diversity sums is not implemented)")

    def _add_diversity(self, rows, recs, pl, p, kind, w, step=None):
        """The twelve diversity columns into ``rows`` (the result rows of plan ``pl``'s records ``recs``)."""
        from sfs2d import diversity as DV
        DV.add_columns(rows, recs, pl.diversity(), p, w, kind, step, (self.pop1_size, self.pop2_size),
                       **({"regions": pl.cfg.regions} if kind == "regions" else {}))

    # ------------------------------------------------------------------ region windows (extension)
    def _no_distributed_regions(self, what):
        if self.distributed:
            raise NotImplementedError(f"{what} is single-GPU (distributed sharding of regions is not implemented)")

    @staticmethod
    def _regions_of(p, regions):
        """``regions`` (a sfs2d.regions.Regions, a BED path, or (chrom_name, first, last[, name]) tuples) as a
        Regions against ``p``'s chromosome names; ValueError for an unknown chromosome, first > last, a duplicate
        row key -- before any GPU work."""
        from sfs2d.regions import Regions
        return Regions.of(p, regions)

    def _region_rows(self, p, pl, rg, recs, fst, diversity):
        """The rows of regions plan ``pl`` (run, alive) from its records."""
        rows = post.region_scan(recs, p, rg, pl.read_fst() if fst else None)
        if diversity:
            self._add_diversity(rows, recs, pl, p, "regions", None)
        return rows

    @staticmethod
    def _null_fill(rows):
        """p_* keys of the rows the null left out (empty regions): None."""
        from sfs2d import null as N
        for row in rows.values():
            for key in N.P_KEYS:
                row.setdefault(key, None)

    def region_scan(self, data_dict, regions, background_chromosome=None, fst=False, diversity=False):
        """The intervals of ``regions`` -- annotated genes, a known inversion, candidate regions, a QTL interval --
        scanned as windows (sfs2d_plan_create_regions).  ``regions``: a
        sfs2d.regions.Regions, a BED file path, or ``(chrom_name, first, last[, name])`` tuples with 1-based
        inclusive positions; they may overlap, nest, repeat and come in any order.  The reference has no such
        scan: its users tile the genome and cut the tiles that overlap each gene out of the table afterwards.
        ``background_chromosome`` None: each chromosome is its own background, the whole chromosome whether or
        not regions cover it (as combined_scan); else that chromosome's SFS for every region (as scan_chooseChr).
        Returns {key: row}, one row PER REGION in the caller's order, the key the region's name or
        "<chrom> <first>-<last>": combined_scan's seven keys, plus "FST" when ``fst`` and the twelve diversity
        columns (per site of the region's own length) when ``diversity``; clean None rules (post.region_scan); a
        region without SNPs has snp_count 0 and None everywhere."""
        self._no_distributed_diversity(diversity)
        self._no_distributed_regions("region_scan")
        p = self._pack(data_dict)
        rg = self._regions_of(p, regions)
        bg = None
        if background_chromosome is not None:
            if background_chromosome not in p.chrom_names:
                raise ValueError(f"Background chromosome {background_chromosome} not found in the data.")
            bg = self._bg_arrays(p, p.chrom_names.index(background_chromosome))
        cfg = self._cfg(p, window_mode=L.WINDOW_BP, fst=bool(fst), regions=rg,
                        bg_mode=L.BG_PER_CHROM if bg is None else L.BG_SUPPLIED)
        eng = self._engine()
        dev = eng.upload(p)
        try:
            pl = eng.plan(dev, cfg)
            try:
                if bg is not None:
                    pl.set_background(*bg)
                pl.run()
                pl.check()
                rows = self._region_rows(p, pl, rg, pl.read(), fst, diversity)
            finally:
                pl.close()
        finally:
            dev.close()
        return rows

    def _multi_scan(self, data_dict, window_sizes, snp_window_sizes, fst, after_run=None, diversity=False, regions=None):
        """multi_scan; ``after_run(p, base plan, [(recs, record labels, rows)])`` is called while the
        plans are alive (scan_pvalues adds its columns there)."""
        self._no_distributed_diversity(diversity)
        if regions is not None:
            self._no_distributed_regions("multi_scan with regions")
        p = self._pack(data_dict)
        rg = None if regions is None else self._regions_of(p, regions)
        bps = sorted(set(int(w) for w in window_sizes))
        snps = [int(x) for x in dict.fromkeys(snp_window_sizes)]
        if not bps and not snps and rg is None:
            return {}
        specs = [("bp", w) for w in bps] + [("snps", S) for S in snps] + ([("regions", None)] if rg is not None else [])
        base_ws = bps[0] if bps else None

        def cfg_of(kind, w):
            if kind == "regions":   # (its Fst needs nothing of the base)
                return self._cfg(p, window_mode=L.WINDOW_BP, bg_mode=L.BG_PER_CHROM, fst=bool(fst), regions=rg)
            bp = kind == "bp"
            want_fst = fst and bp and base_ws is not None   # (the library refuses what it cannot attach)
            return self._cfg(p, window_mode=L.WINDOW_BP if bp else L.WINDOW_SNPS, window=w,
                             bg_mode=L.BG_PER_CHROM, prev_extra=bp, fst=want_fst)
        eng = self._engine()
        dev = eng.upload(p)
        out = {}
        try:
            base = eng.plan(dev, cfg_of(*specs[0]))
            try:
                plans = [base]
                for sp in specs[1:]:
                    c = cfg_of(*sp)
                    try:
                        plans.append(base.attach(c))
                    except L.Sfs2dError:
                        if not c.fst:
                            raise
                        c.fst = False   # Fst for this window size from its own plan below
                        plans.append(base.attach(c))
                base.run()
                base.check()
                items = []
                for (kind, w), pl in zip(specs, plans):
                    pl.check()
                    recs = pl.read()
                    if kind == "regions":
                        out["regions"] = self._region_rows(p, pl, rg, recs, fst, diversity)
                        if after_run is not None:
                            items.append((recs, post.region_labels(recs, rg), out["regions"]))
                        continue
                    if kind == "bp":
                        out[w] = post.combined_scan(recs, p, w, post.num_slots(recs))
                        if pl.cfg.fst:
                            out.setdefault("fst", {})[w] = post.window_fst_labels(recs, pl.read_fst(), p, w, True)
                    else:
                        out[f"{w}snps"] = post.bysnp_scan(recs, p, w, with_diff=True, final_warning=False)
                    if diversity:
                        self._add_diversity(out[w if kind == "bp" else f"{w}snps"], recs, pl, p, kind, w)
                    if after_run is not None:
                        items.append((recs, post.record_labels(recs, p, kind, w), out[w if kind == "bp" else f"{w}snps"]))
                if after_run is not None:
                    after_run(p, base, items)
                    if rg is not None:
                        self._null_fill(out["regions"])
            finally:
                base.close()
        finally:
            dev.close()
        if fst:
            for w in bps:
                if w not in out.get("fst", {}):
                    out.setdefault("fst", {})[w] = self.window_fst(p, window_size=w)
        return out

    # ------------------------------------------------------------------ sliding windows (extension)
    @staticmethod
    def _check_steps(window_sizes, step_size):
        """The sliding geometry's rules (sfs2d_plan_create_sliding), checked before any GPU work."""
        step = int(step_size)
        if step < 1:
            raise ValueError(f"step_size must be >= 1, got {step_size}")
        for w in window_sizes:
            if int(w) < step or int(w) % step != 0:
                raise ValueError(f"step_size {step} does not divide window size {w}")
            if int(w) // step > 64:
                raise ValueError(f"window size {w} is more than 64 steps of {step}")
        return step

    def sliding_scan(self, data_dict, window_size, step_size, background_chromosome=None, fst=False, diversity=False):
        """Overlapping fixed-bp windows: ``window_size`` bp advanced by ``step_size`` bp (a divisor of the
        window, at most 64 steps per window; sfs2d_plan_create_sliding).  The reference has no such scan:
        its script scans at 20 kb and at 500 kb and compares (twoDSFS_class.py:1923-1932) because a signal on
        an edge of its disjoint windows is split between two of them.  ``background_chromosome`` None: each
        chromosome is its own background (as combined_scan); else that chromosome's SFS for every window (as
        scan_chooseChr).  Returns {"<chrom> <start>-<end>": row} per non-empty window with combined_scan's
        seven keys, plus "FST" (Hudson's, as window_fst) when ``fst`` and the twelve diversity columns
        (``window_diversity``) when ``diversity``; clean None rules (post.sliding_scan)."""
        self._no_distributed_diversity(diversity)
        if self.distributed:
            raise NotImplementedError("sliding_scan is single-GPU (distributed sharding of sliding windows is not implemented)")
        ws = int(window_size)
        step = self._check_steps([ws], step_size)
        p = self._pack(data_dict)
        bg = None
        if background_chromosome is not None:
            if background_chromosome not in p.chrom_names:
                raise ValueError(f"Background chromosome {background_chromosome} not found in the data.")
            bg = self._bg_arrays(p, p.chrom_names.index(background_chromosome))
        cfg = self._cfg(p, window_mode=L.WINDOW_BP, window=ws, fst=bool(fst), step=step,
                        bg_mode=L.BG_PER_CHROM if bg is None else L.BG_SUPPLIED)
        eng = self._engine()
        dev = eng.upload(p)
        try:
            pl = eng.plan(dev, cfg)
            try:
                if bg is not None:
                    pl.set_background(*bg)
                pl.run()
                pl.check()
                recs = pl.read()
                f = pl.read_fst() if fst else None
                rows = post.sliding_scan(recs, p, ws, step, f)
                if diversity:
                    self._add_diversity(rows, recs, pl, p, "bp", ws, step)
            finally:
                pl.close()
        finally:
            dev.close()
        return rows

    def multi_sliding_scan(self, data_dict, window_sizes, step_size, fst=False, diversity=False, regions=None):
        """sliding_scan (per-chromosome backgrounds) at every size in ``window_sizes`` with one step, from
        ONE upload and one k_prep pass: the smallest window is a sliding plan of its own, the others are
        attached to it (sfs2d_plan_attach_sliding).  Returns {window_size: sliding_scan rows}.  A window the
        step does not divide raises ValueError before any GPU work.  ``diversity``, ``regions``: as in multi_scan."""
        if regions is None:
            return self._multi_sliding_scan(data_dict, window_sizes, step_size, fst, diversity=diversity)
        return self._multi_sliding_scan(data_dict, window_sizes, step_size, fst, diversity=diversity, regions=regions)

    def _multi_sliding_scan(self, data_dict, window_sizes, step_size, fst, after_run=None, diversity=False, regions=None):
        """multi_sliding_scan, with ``after_run`` as in _multi_scan."""
        self._no_distributed_diversity(diversity)
        if self.distributed:
            raise NotImplementedError("multi_sliding_scan is single-GPU (distributed sharding of sliding windows is not implemented)")
        wss = sorted(set(int(w) for w in window_sizes))
        step = self._check_steps(wss, step_size)
        if not wss and regions is None:
            return {}
        p = self._pack(data_dict)
        rg = None if regions is None else self._regions_of(p, regions)
        rcfg = None if rg is None else self._cfg(p, window_mode=L.WINDOW_BP, bg_mode=L.BG_PER_CHROM, fst=bool(fst), regions=rg)

        def cfg_of(w):
            return self._cfg(p, window_mode=L.WINDOW_BP, window=w, bg_mode=L.BG_PER_CHROM, fst=bool(fst), step=step)
        eng = self._engine()
        dev = eng.upload(p)
        out = {}
        try:
            base = eng.plan(dev, cfg_of(wss[0]) if wss else rcfg)
            try:
                plans = [base] + [base.attach(cfg_of(w)) for w in wss[1:]]
                rpl = None if rg is None else base.attach(rcfg) if wss else base
                base.run()
                base.check()
                items = []
                for w, pl in zip(wss, plans):
                    pl.check()
                    recs = pl.read()
                    out[w] = post.sliding_scan(recs, p, w, step, pl.read_fst() if fst else None)
                    if diversity:
                        self._add_diversity(out[w], recs, pl, p, "bp", w, step)
                    if after_run is not None:
                        items.append((recs, post.record_labels(recs, p, "bp", w, step), out[w]))
                if rpl is not None:
                    rpl.check()
                    recs = rpl.read()
                    out["regions"] = self._region_rows(p, rpl, rg, recs, fst, diversity)
                    if after_run is not None:
                        items.append((recs, post.region_labels(recs, rg), out["regions"]))
                if after_run is not None:
                    after_run(p, base, items)
                    if rg is not None:
                        self._null_fill(out["regions"])
            finally:
                base.close()
        finally:
            dev.close()
        return out

    # ------------------------------------------------------------------ bootstrap null (extension)
    def _null_columns(self, p, base, items, replicates, seed, sizes, pool=None, block=1):
        """Add the six p_* keys to every row of ``items`` ([(records, record labels, rows)] of plans that
        share ``base``'s data and tables): one null run on ``base`` over the union of the (pool, size class)
        pairs of all windows, the exceedance counts taken on the device (sfs2d.null.pvalues_device).
        pool: the background chromosome of every window (None: each window's own chromosome); block: the
        null's block length (1: single SNPs)."""
        import torch
        from sfs2d import null as N
        sel = []
        for recs, labels, rows in items:
            idx = np.array([i for i, lb in enumerate(labels) if lb is not None and lb in rows], np.int64)
            sel.append((recs[idx], [labels[i] for i in idx], rows))
        obs = np.concatenate([s[0] for s in sel]) if sel else np.zeros(0, L.WINDOW_DTYPE)
        if len(obs) == 0:
            return
        m = obs["end"].astype(np.int64) - obs["begin"].astype(np.int64)
        classes = N.size_classes(m, sizes)
        pools = obs["chrom"].astype(np.int64) if pool is None else np.full(len(obs), int(pool), np.int64)
        tasks = sorted(set(zip(pools.tolist(), classes.tolist())))
        R = int(replicates)
        eng = base.eng
        buf = torch.empty(len(tasks) * R * L.WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=f"cuda:{self.device}")
        torch.cuda.synchronize(buf.device)   # (the engine's stream is ordered against nothing of torch's)
        base.null_run(tasks, R, seed, out_dev_ptr=buf.data_ptr(), block=block)
        h = eng.stream_handle()
        if h:
            torch.cuda.ExternalStream(h, device=buf.device).synchronize()
        else:
            torch.cuda.synchronize(buf.device)
        pv = N.pvalues_device(obs, classes, buf, tasks, R, pools)
        k = 0
        for recs, labels, rows in sel:
            for lb in labels:
                for key in N.P_KEYS:
                    v = pv[key][k]
                    rows[lb][key] = None if np.isnan(v) else float(v)
                k += 1

    @staticmethod
    def _null_block(block):
        """scan_pvalues' ``block`` as a block length: None -> 1, "window" -> 2**32 - 1 (longer than any class),
        an int in [1, 2**32) -> itself."""
        if block is None:
            return 1
        if isinstance(block, str):
            if block != "window":
                raise ValueError(f"block must be None, an int >= 1 or 'window', got {block!r}")
            return 0xFFFFFFFF
        if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or not 1 <= int(block) < (1 << 32):
            raise ValueError(f"block must be None, an int in [1, 2**32) or 'window', got {block!r}")
        return int(block)

    def scan_pvalues(self, data_dict, window_sizes=(), snp_window_sizes=(), step_size=None,
                     background_chromosome=None, replicates=999, seed=0, sizes=None, fst=False, block=None,
                     diversity=False, regions=None):
        """The scans of ``multi_scan`` (``step_size`` given: ``multi_sliding_scan``) with a bootstrap p-value
        beside every statistic: each row additionally holds p_T2D, p_T1D_pop1, p_T1D_pop2, p_new_term_pop1,
        p_new_term_pop2 and p_T2D_diff -- the share of ``replicates`` windows of the same number of SNPs
        (rounded up to a size class, sfs2d.null.size_classes; ``sizes``: None, "exact" or a list) drawn with
        replacement from the window's background chromosome whose statistic is at least the window's
        (definition, what the null does not model).  The p-values of the derived
        terms are formed from the window's own three T's (None when one is None), not from
        combined_scan's carried values.  One null run per call serves every window size.
        ``block``: None or 1 draws single SNPs (no linkage: p-values of linked data are anti-conservative);
        an int b > 1 draws runs of b consecutive SNPs of the (circular) chromosome, the last one cut at the
        class size; "window" makes every run as long as its class -- a random placement of a window of
        that many SNPs on the chromosome ("blocks").
        ``background_chromosome``: one window size, scanned as scan_chooseChr (or scan_chooseChr_bySNPs for a
        SNP-count size, sliding_scan with ``step_size``) does; that chromosome is every window's pool; the
        result is {size: rows}.  ``diversity``: every row also holds the twelve diversity columns
        (``window_diversity``; they get no p-values).  ``regions`` (as in ``region_scan``): the per-region rows as
        well, under the "regions" key, from a regions plan attached to the same base; a region's pool is its
        chromosome (or ``background_chromosome``, then without window sizes: {"regions": rows}), its m its SNP
        count end - begin through the same size classes, blocks and p-value rule; an empty region's p-values are
        None.  Not in the reference (it thresholds by SNP-count quantile and top 1 % in R,
        ECBstats_plots.R:45-50, 147-219)."""
        self._no_distributed_diversity(diversity)
        if self.distributed:
            raise NotImplementedError("scan_pvalues is single-GPU (distributed sharding of the null is not implemented)")
        if int(replicates) < 1:
            raise ValueError(f"replicates must be >= 1, got {replicates}")
        if sizes is not None and sizes != "exact":
            sizes = sorted(int(x) for x in sizes)
        block = self._null_block(block)
        rkw = {} if regions is None else {"regions": regions}

        def hook(pool=None):
            return lambda p, base, items: self._null_columns(p, base, items, replicates, seed, sizes, pool, block)
        if background_chromosome is None:
            if step_size is None:
                return self._multi_scan(data_dict, window_sizes, snp_window_sizes, fst, hook(), diversity=diversity, **rkw)
            if len(tuple(snp_window_sizes)):
                raise ValueError("step_size applies to fixed-bp windows: not with snp_window_sizes")
            return self._multi_sliding_scan(data_dict, window_sizes, step_size, fst, hook(), diversity=diversity, **rkw)
        # one chromosome as every window's background (and pool)
        bps, snps = [int(w) for w in window_sizes], [int(w) for w in snp_window_sizes]
        if regions is not None:
            return self._region_pvalues(data_dict, regions, bps, snps, step_size, background_chromosome, replicates,
                                        seed, sizes, fst, block, diversity)
        if len(bps) + len(snps) != 1:
            raise ValueError("background_chromosome takes exactly one window size")
        if step_size is not None and snps:
            raise ValueError("step_size applies to fixed-bp windows: not with snp_window_sizes")
        if fst and step_size is None:
            raise ValueError("fst with background_chromosome needs step_size (scan_chooseChr has no Fst)")
        p = self._pack(data_dict)
        if background_chromosome not in p.chrom_names:
            raise ValueError(f"Background chromosome {background_chromosome} not found in the data.")
        bgc = p.chrom_names.index(background_chromosome)
        bg = self._bg_arrays(p, bgc)
        step = None if step_size is None else self._check_steps(bps, step_size)
        if snps:   # scan_chooseChr_bySNPs: the normalised background
            bg = tuple(np.array(self._normalize_values(np.asarray(b).ravel().tolist())) for b in bg)
        w = (bps or snps)[0]
        cfg = self._cfg(p, window_mode=L.WINDOW_SNPS if snps else L.WINDOW_BP, window=w, bg_mode=L.BG_SUPPLIED,
                        step=step, fst=bool(fst))
        eng = self._engine()
        dev = eng.upload(p)
        try:
            pl = eng.plan(dev, cfg)
            try:
                pl.set_background(*bg)
                pl.run()
                pl.check()
                recs = pl.read()
                if snps:
                    rows = post.bysnp_scan(recs, p, w, with_diff=False, final_warning=True)
                elif step is not None:
                    rows = post.sliding_scan(recs, p, w, step, pl.read_fst() if fst else None)
                else:
                    rows = post.fixed_bg_scan(recs, p, w, post.num_slots(recs))
                labels = post.record_labels(recs, p, "snps" if snps else "bp", w, step)
                if diversity:
                    self._add_diversity(rows, recs, pl, p, "snps" if snps else "bp", w, step)
                self._null_columns(p, pl, [(recs, labels, rows)], replicates, seed, sizes, pool=bgc, block=block)
            finally:
                pl.close()
        finally:
            dev.close()
        return {(f"{w}snps" if snps else w): rows}

    def _region_pvalues(self, data_dict, regions, bps, snps, step_size, background_chromosome, replicates, seed,
                        sizes, fst, block, diversity):
        """scan_pvalues with ``regions`` and one chromosome as every region's background and pool."""
        if bps or snps or step_size is not None:
            raise ValueError("regions with background_chromosome take no window sizes and no step_size")
        p = self._pack(data_dict)
        rg = self._regions_of(p, regions)
        if background_chromosome not in p.chrom_names:
            raise ValueError(f"Background chromosome {background_chromosome} not found in the data.")
        bgc = p.chrom_names.index(background_chromosome)
        bg = self._bg_arrays(p, bgc)
        cfg = self._cfg(p, window_mode=L.WINDOW_BP, bg_mode=L.BG_SUPPLIED, fst=bool(fst), regions=rg)
        eng = self._engine()
        dev = eng.upload(p)
        try:
            pl = eng.plan(dev, cfg)
            try:
                pl.set_background(*bg)
                pl.run()
                pl.check()
                recs = pl.read()
                rows = self._region_rows(p, pl, rg, recs, fst, diversity)
                self._null_columns(p, pl, [(recs, post.region_labels(recs, rg), rows)], replicates, seed, sizes,
                                   pool=bgc, block=block)
                self._null_fill(rows)
            finally:
                pl.close()
        finally:
            dev.close()
        return {"regions": rows}

    # ------------------------------------------------------------------ Fst (extension)
    def window_fst(self, data_dict, window_size=None, snp_window_size=None):
        """Hudson's Fst per window (not in the reference, whose published FST column is pixy's
        Weir-Cockerham joined in R, ECBstats_plots.R:16-41): {label: Fst or None}, labels as
        combined_scan (fixed bp, ``window_size``) or scan_perChr_bySNPs (``snp_window_size``) emit
        them.  Computed by k_prep on the GPU ("Fst")."""
        p = self._pack(data_dict)
        if (window_size is None) == (snp_window_size is None):
            raise ValueError("give exactly one of window_size / snp_window_size")
        bp = window_size is not None
        cfg = self._cfg(p, window_mode=L.WINDOW_BP if bp else L.WINDOW_SNPS,
                        window=int(window_size if bp else snp_window_size), bg_mode=L.BG_PER_CHROM, fst=True)
        eng = self._engine()
        dev = eng.upload(p)
        try:
            pl = eng.plan(dev, cfg)
            try:
                pl.run()
                pl.check()
                recs, fst = pl.read(), pl.read_fst()
            finally:
                pl.close()
        finally:
            dev.close()
        return post.window_fst_labels(recs, fst, p, int(window_size if bp else snp_window_size), bp)

    # ------------------------------------------------------------------ diversity (extension)
    def window_diversity(self, data_dict, window_size=None, snp_window_size=None, step_size=None):
        """What kind of window a T2D / Fst peak is: per window {label: {pi_pop1, pi_pop2, dxy, da, theta_w_pop1,
        theta_w_pop2, S_pop1, S_pop2, S_full_pop1, S_full_pop2, tajima_d_pop1, tajima_d_pop2}}, labels as
        combined_scan (``window_size``; sliding_scan with ``step_size``) or scan_perChr_bySNPs
        (``snp_window_size``) emit them.  Not in the reference (its users join pixy's or scikit-allel's columns
        by window label).  The sums are taken on the GPU over the SNPs of each window's 2D SFS (k_div_win;
        DESIGN.md section 15, sfs2d.diversity): pi, dxy, da = dxy - (pi1 + pi2) / 2 and Watterson's theta are
        per site -- divided by the window size in bp (every site of a fixed-bp window is taken as callable: a
        SNP-only VCF knows nothing else) or, for SNP-count windows, by last position - first position + 1; S is
        the number of segregating sites; Tajima's D rests on the S_full SNPs that are fully called in the
        population (D is defined for one sample size) and is None without any, or for fewer than 2 individuals."""
        self._no_distributed_diversity(True)
        p = self._pack(data_dict)
        if (window_size is None) == (snp_window_size is None):
            raise ValueError("give exactly one of window_size / snp_window_size")
        bp = window_size is not None
        if step_size is not None and not bp:
            raise ValueError("step_size applies to fixed-bp windows: not with snp_window_size")
        w = int(window_size if bp else snp_window_size)
        step = None if step_size is None else self._check_steps([w], step_size)
        cfg = self._cfg(p, window_mode=L.WINDOW_BP if bp else L.WINDOW_SNPS, window=w, bg_mode=L.BG_PER_CHROM, step=step)
        from sfs2d import diversity as DV
        eng = self._engine()
        dev = eng.upload(p)
        try:
            pl = eng.plan(dev, cfg)
            try:
                pl.run()
                pl.check()
                recs, div = pl.read(), pl.diversity()
            finally:
                pl.close()
        finally:
            dev.close()
        return DV.rows(recs, div, p, w, "bp" if bp else "snps", step, (self.pop1_size, self.pop2_size))

    # ------------------------------------------------------------------ window spectra (extension)
    def _no_distributed_spectra(self, what):
        if self.distributed:
            raise NotImplementedError(f"{what} is single-GPU (distributed sharding of the window spectra is not implemented)")

    def _spectra_cfg(self, p, window_size, snp_window_size, step_size, regions, **kw):
        """(cfg, kind, w, step, Regions) of the one window geometry given."""
        given = [x is not None for x in (window_size, snp_window_size, regions)]
        if sum(given) != 1:
            raise ValueError("give exactly one of window_size / snp_window_size / regions")
        if step_size is not None and window_size is None:
            raise ValueError("step_size applies to fixed-bp windows: give window_size")
        if regions is not None:
            rg = self._regions_of(p, regions)
            return self._cfg(p, window_mode=L.WINDOW_BP, regions=rg, **kw), "regions", None, None, rg
        bp = window_size is not None
        w = int(window_size if bp else snp_window_size)
        step = None if step_size is None else self._check_steps([w], step_size)
        cfg = self._cfg(p, window_mode=L.WINDOW_BP if bp else L.WINDOW_SNPS, window=w, step=step, **kw)
        return cfg, "bp" if bp else "snps", w, step, None

    def _check_project(self, project):
        """(m1, m2) of a ``project=`` argument, ValueError when it is no pair within [2, 2 pop_size]."""
        try:
            m1, m2 = (int(x) for x in project)
        except (TypeError, ValueError):
            raise ValueError(f"project: a pair (m1, m2) of haploid sample sizes, got {project!r}") from None
        if not (2 <= m1 <= 2 * self.pop1_size and 2 <= m2 <= 2 * self.pop2_size):
            raise ValueError(f"project: ({m1}, {m2}) outside [2, {2 * self.pop1_size}] x [2, {2 * self.pop2_size}]")
        return m1, m2

    def _projected_entry(self, grid, used, dropped):
        """One projected group as the spectra methods return it: folded when the object folds."""
        from sfs2d import spectra as SP
        s1, s2 = SP.projected_marginals(grid)
        if self.fold:
            grid, s1, s2 = SP.fold_projected(grid), SP.fold1d_projected(s1), SP.fold1d_projected(s2)
        return {"sfs2d": grid, "sfs1d_pop1": s1, "sfs1d_pop2": s2, "n_used": int(used), "n_dropped": int(dropped)}

    def window_spectra(self, data_dict, window_size=None, snp_window_size=None, step_size=None, regions=None,
                       select=None, project=None):
        """The spectra themselves of a scan's windows, where the scans return them reduced to T2D / T1D:
        {label: {"sfs2d": int64 grid (2 pop1_size + 1, 2 pop2_size + 1), "sfs1d_pop1", "sfs1d_pop2": folded 1D
        spectra}}, labels as combined_scan (``window_size``; sliding_scan with ``step_size``), scan_perChr_bySNPs
        (``snp_window_size``) or region_scan (``regions``: one entry per region, an empty region all zero) emit them.
        ``select``: a list of those labels (None: every window), one entry each, in that order.  The grid is
        calculate_2d_sfs over the window under the object's filters and fold -- bin (0, 0) is 0, the last bin is
        counted; the 1D spectra hold the inner bins 1 .. pop_size - 1 that T1D reads, entries 0 and pop_size are 0.
        Summed on the GPU from the data the scan holds (k_spec_win).  The
        reference cuts the windows' SNPs into new VCFs and reads them again (sims_scan.py:726-936).
        ``project`` = (m1, m2): the spectra projected down hypergeometrically to m1 / m2 haploid samples
        (k_proj_win), what a model fit takes when calls are missing: "sfs2d" is then a
        float64 (m1 + 1, m2 + 1) grid of the SNPs called in at least m_k alleles of both populations, "sfs1d_pop1" /
        "sfs1d_pop2" its two marginals (m_k + 1 entries, every bin), all three folded when the object folds (a tie
        of the joint fold stays where it is; dadi averages ties), and "n_used" / "n_dropped" count the window's SNPs
        that reached the sample sizes and those that did not."""
        self._no_distributed_spectra("window_spectra")
        if project is not None:
            project = self._check_project(project)
        p = self._pack(data_dict)
        cfg, kind, w, step, rg = self._spectra_cfg(p, window_size, snp_window_size, step_size, regions,
                                                   bg_mode=L.BG_PER_CHROM)
        from sfs2d import spectra as SP
        eng = self._engine()
        dev = eng.upload(p)
        try:
            pl = eng.plan(dev, cfg)
            try:
                pl.run()
                pl.check()
                recs = pl.read()
                if rg is not None:   # (every region has an entry, in the caller's order)
                    index = {k: int(s) for k, s in zip(rg.keys(), rg.slot.tolist())}
                else:
                    index = {lb: i for i, lb in enumerate(post.record_labels(recs, p, kind, w, step)) if lb is not None}
                labels = list(index) if select is None else list(select)
                for lb in labels:
                    if lb not in index:
                        raise ValueError(f"window_spectra: no window labelled {lb!r}")
                if project is not None:
                    proj = pl.project(*project, [index[lb] for lb in labels], np.arange(len(labels), dtype=np.int32),
                                      max(1, len(labels)))
                else:
                    rows = pl.spectra([index[lb] for lb in labels], np.arange(len(labels), dtype=np.int32),
                                      max(1, len(labels)))
            finally:
                pl.close()
        finally:
            dev.close()
        if project is not None:
            return {lb: self._projected_entry(g, u, d) for lb, g, u, d in zip(labels, *proj)}
        out = {}
        for lb, row in zip(labels, rows):
            g, f1, f2 = SP.split_row(row, self.pop1_size, self.pop2_size)
            out[lb] = {"sfs2d": g.copy(), "sfs1d_pop1": f1.copy(), "sfs1d_pop2": f2.copy()}
        return out

    @staticmethod
    def _clean_rows(recs, labels, fst=None):
        """{label: combined_scan's seven keys (+ "FST")} of the labelled records, with sliding_scan's clean None
        rules (no stale carry, no final block, no TypeError)."""
        rows = {}
        for i, (r, lb) in enumerate(zip(recs, labels)):
            if lb is None:
                continue
            T2D, T1, T2 = post._v(r, 2), post._v(r, 1), post._v(r, 0)
            row = {"snp_count": int(r["snp_count"]), "T2D": T2D, "T1D_pop1": T1, "T1D_pop2": T2,
                   "new_term_pop1": None if T2D is None or T1 is None else T2D - T1,
                   "new_term_pop2": None if T2D is None or T2 is None else T2D - T2,
                   "T2D_diff": None if T2D is None or T1 is None or T2 is None else T2D - (T1 + T2) / 2}
            if fst is not None:
                row["FST"] = None if i >= len(fst) or np.isnan(fst[i]) else float(fst[i])
            rows[lb] = row
        return rows

    def outlier_spectra(self, data_dict, window_size=None, key="T2D", q=0.99, fst=False, snp_window_size=None,
                        step_size=None, background_chromosome=None, project=None):
        """The joint spectrum of a scan's outlier windows beside its background, and which bins drive T2D: the
        windows whose ``key`` (T2D, T1D_pop1, T1D_pop2, new_term_pop1, new_term_pop2, T2D_diff, snp_count; or FST
        with ``fst``) is in the top 1 - ``q`` of the scan (sfs2d.spectra.select_top: value >= the ``q`` quantile
        of the windows that have one; the statistics with sliding_scan's clean None rules), pooled into ONE
        spectrum on the GPU from the data the scan holds.  Windows as in ``window_spectra`` (``window_size``,
        with ``step_size`` sliding; or ``snp_window_size``); ``background_chromosome`` as in sliding_scan.
        Returns {"labels": the selected labels in scan order, "foreground": the pooled int64 grid,
        "sfs1d_pop1" / "sfs1d_pop2": the pooled folded 1D spectra, "background": the pooled background grid --
        the sum of the whole-chromosome grids of the chromosomes that hold a selected window, or
        ``background_chromosome``'s --, "background_chromosomes": their names, "residuals":
        sfs2d.spectra.residuals(foreground, background), "T2D": the pooled foreground's T2D against that
        background (the sum of the residual terms; None when either is empty)}.  On sliding windows the pool is a
        sum over windows, not the spectrum of their union: a SNP in two selected windows is counted twice.  The
        reference merges the outlier windows' VCFs with an outside tool, reads them again and subtracts the
        normalised spectra (sims_scan.py:726-936).
        ``project`` = (m1, m2): the pooled foreground and the background both projected down to m1 / m2 haploid
        samples on the GPU (``window_spectra``'s ``project``; the background through whole-chromosome entries of the
        same call, under the scan's own membership), float64 grids folded when the object folds; the residuals
        and the pooled T2D come from them.  Added keys: "n_used" / "n_dropped" of the foreground,
        "background_n_used" / "background_n_dropped"."""
        self._no_distributed_spectra("outlier_spectra")
        if project is not None:
            project = self._check_project(project)
        if key == "FST" and not fst:
            raise ValueError("key 'FST' needs fst=True")
        p = self._pack(data_dict)
        bg = None
        if background_chromosome is not None:
            if background_chromosome not in p.chrom_names:
                raise ValueError(f"Background chromosome {background_chromosome} not found in the data.")
            bg = self._bg_arrays(p, p.chrom_names.index(background_chromosome))
        cfg, kind, w, step, _ = self._spectra_cfg(p, window_size, snp_window_size, step_size, None, fst=bool(fst),
                                                  bg_mode=L.BG_PER_CHROM if bg is None else L.BG_SUPPLIED)
        from sfs2d import spectra as SP
        eng = self._engine()
        dev = eng.upload(p)
        try:
            pl = eng.plan(dev, cfg)
            try:
                if bg is not None:
                    pl.set_background(*bg)
                pl.run()
                pl.check()
                recs = pl.read()
                labels = post.record_labels(recs, p, kind, w, step)
                rows = self._clean_rows(recs, labels, pl.read_fst() if fst else None)
                top = SP.select_top(rows, key, q)
                index = {lb: i for i, lb in enumerate(labels) if lb is not None}
                sel = [index[lb] for lb in top]
                chroms = ([p.chrom_names.index(background_chromosome)] if bg is not None
                          else sorted(set(int(recs[i]["chrom"]) for i in sel)))
                if project is not None:   # group 0: the pooled windows; group 1: the chromosomes, whole
                    proj = pl.project(*project, sel + [-(c + 1) for c in chroms], [0] * len(sel) + [1] * len(chroms), 2)
                    bg_names = [p.chrom_names[c] for c in chroms]
                else:
                    row = pl.spectra(sel, np.zeros(len(sel), np.int32), 1)[0]
                    if bg is not None:
                        bg_grid, bg_names = np.asarray(bg[0], np.int64), [background_chromosome]
                    else:
                        bg_names = [p.chrom_names[c] for c in chroms]
                        bg_grid = sum(np.asarray(eng.bg_hist(dev, cfg, c)[0], np.int64) for c in chroms)
            finally:
                pl.close()
        finally:
            dev.close()
        if project is not None:
            f, b = (self._projected_entry(g, u, d) for g, u, d in zip(*proj))
            res = SP.residuals(f["sfs2d"], b["sfs2d"])
            return {"labels": top, "foreground": f["sfs2d"], "sfs1d_pop1": f["sfs1d_pop1"], "sfs1d_pop2": f["sfs1d_pop2"],
                    "background": b["sfs2d"], "background_chromosomes": bg_names, "residuals": res,
                    "T2D": SP.pooled_t2d(res), "n_used": f["n_used"], "n_dropped": f["n_dropped"],
                    "background_n_used": b["n_used"], "background_n_dropped": b["n_dropped"]}
        g, f1, f2 = SP.split_row(row, self.pop1_size, self.pop2_size)
        res = SP.residuals(g, bg_grid)
        return {"labels": top, "foreground": g.copy(), "sfs1d_pop1": f1.copy(), "sfs1d_pop2": f2.copy(),
                "background": bg_grid, "background_chromosomes": bg_names, "residuals": res, "T2D": SP.pooled_t2d(res)}

    # ------------------------------------------------------------------ projected scan (extension)
    def projected_scan(self, data_dict, project, window_size=None, snp_window_size=None, step_size=None, regions=None,
                       background_chromosome=None, replicates=None, seed=0):
        """T2D and T1D of every window at a common sample size: the scan's statistics from spectra projected down
        hypergeometrically to ``project`` = (m1, m2) haploid samples, each window against its chromosome projected
        the same way (``background_chromosome``: that chromosome for every window, as scan_chooseChr).  The scans
        bin a SNP by its raw alt count whatever its called count, so a window where calls are missing -- low
        coverage, repeats, one population sequenced worse -- has its spectrum pushed toward the low bins and T2D
        reports that as signal; here only SNPs called in at least m_k alleles of both populations count, each
        spread over the bins its subsamples fall in (k_proj_scan, on the GPU).  Windows as in
        ``window_spectra``: ``window_size`` (with ``step_size`` sliding), ``snp_window_size`` or ``regions``, labels
        as the corresponding scans emit them.  Returns {label: {snp_count, n_used, n_dropped, T2D_proj,
        T1D_pop1_proj, T1D_pop2_proj, new_term_pop1_proj, new_term_pop2_proj, T2D_diff_proj}}
        (sfs2d.spectra.project_scan_rows): None for an empty foreground or background, +inf where the window
        touches a bin its background lacks.  The statistic is the closed form 2 sum x_k (ln(x_k / N) - ln(b_k /
        B)) over the inner bins; the reference's exact 0.0 for proportional spectra is not reproduced.  The
        reference has no projection.
        ``replicates`` = R: every row gains p_T2D_proj, p_T1D_pop1_proj, p_T1D_pop2_proj, p_new_term_pop1_proj,
        p_new_term_pop2_proj, p_T2D_diff_proj and n_thin (sfs2d.projnull): the projected T
        still grows as a window's called counts approach the projection, so each window is judged against R
        replicates of itself in which every used SNP is redrawn among the used SNPs of its chromosome with the
        same called counts (k_proj_null, on the GPU; ``seed`` the draws'); p = (1 + exceedances) / (R + 1), None
        where the statistic is None; n_thin counts the window's used SNPs whose stratum holds fewer than 8 SNPs
        (redrawn from almost nothing).  Not with ``background_chromosome`` (a foreign pool can have empty strata)
        nor distributed: NotImplementedError."""
        if replicates is not None:
            if background_chromosome is not None:
                raise NotImplementedError("projected_scan: replicates with background_chromosome (the null draws from "
                                          "each window's own chromosome; a foreign pool can have empty strata)")
            if getattr(self, "distributed", False):
                raise NotImplementedError("projected_scan: replicates on a distributed object")
            if isinstance(replicates, bool) or int(replicates) != replicates or int(replicates) < 1:
                raise ValueError(f"projected_scan: replicates must be an integer >= 1, got {replicates!r}")
            replicates = int(replicates)
        self._no_distributed_spectra("projected_scan")
        project = self._check_project(project)
        p = self._pack(data_dict)
        bg_chrom = None
        if background_chromosome is not None:
            if background_chromosome not in p.chrom_names:
                raise ValueError(f"Background chromosome {background_chromosome} not found in the data.")
            bg_chrom = p.chrom_names.index(background_chromosome)
        cfg, kind, w, step, rg = self._spectra_cfg(p, window_size, snp_window_size, step_size, regions,
                                                   bg_mode=L.BG_PER_CHROM)
        from sfs2d import spectra as SP
        eng = self._engine()
        dev = eng.upload(p)
        try:
            pl = eng.plan(dev, cfg)
            try:
                pl.run()
                pl.check()
                recs = pl.read()
                stats = pl.project_scan(*project, bg_chrom)
                if replicates is not None:
                    null, thin = pl.project_null(*project, replicates, seed)
            finally:
                pl.close()
        finally:
            dev.close()
        if rg is not None:   # (one row per region, in the caller's order)
            order = rg.slot.tolist()
            rows, labels = SP.project_scan_rows(recs[order], stats[order], list(rg.keys())), list(rg.keys())
        else:
            order = None
            labels = post.record_labels(recs, p, kind, w, step)
            rows = SP.project_scan_rows(recs, stats, labels)
        if replicates is not None:
            from sfs2d import projnull as PN
            pv = PN.project_pvalues(stats, null, replicates)
            if order is not None:
                pv, thin = {k: v[order] for k, v in pv.items()}, thin[order]
            PN.add_pvalue_columns(rows, labels, pv, thin)
        return rows

    # ------------------------------------------------------------------ SFS primitives
    def calculate_2d_sfs(self, data_dict):
        """2D SFS dict over the grid (140-232), accumulated on the GPU (distributed: every rank a slice
        of the SNPs, one device all-reduce -- the genome-wide background of the reference script,
        1970-1983, from sharded data)."""
        self.data_dict = data_dict
        p = self._pack(data_dict)
        n1, n2 = 2 * self.pop1_size, 2 * self.pop2_size
        if p.n == 0:
            return {(i, j): 0 for i in range(n1 + 1) for j in range(n2 + 1)}
        h2, _, _ = self._hist(p, self._cfg(p), -1)
        return {(i, j): int(h2[i, j]) for i in range(n1 + 1) for j in range(n2 + 1)}

    def calculate_1d_sfs(self, data_dict, pop, pop_size, start_position, end_position, variant_type):
        """Unfolded 1D SFS dict of raw alt counts (398-444), accumulated on the GPU."""
        self.data_dict = data_dict
        self.pop = pop
        self.pop_size = pop_size
        self.start_position = start_position
        self.end_position = end_position
        self.variant_type = variant_type
        p = self._pack(data_dict, pop1=pop, pop2=pop).single_pop(pop)
        if p.n == 0:
            return {i: 0 for i in range(2 * pop_size + 1)}
        ann = -1
        if variant_type is not None:
            ann = p.ann_names.index(variant_type) if variant_type in p.ann_names else _NO_ANN
        cfg = ScanConfig(n1p=pop_size, n2p=pop_size, fold=False, ann_want=ann,
                         start_position=None if start_position is None else int(start_position),
                         end_position=None if end_position is None else int(end_position))
        _, u1, _ = self._hist(p, cfg, -1)
        return {i: int(u1[i]) for i in range(2 * pop_size + 1)}

    def fold_1d_sfs(self, sfs_dict):
        """446-463: minor = min(f, F - f) with F = max key."""
        num_chromosomes = max(sfs_dict.keys())
        folded = {}
        for freq, count in sfs_dict.items():
            m = min(freq, num_chromosomes - freq)
            folded[m] = folded[m] + count if m in folded else count
        return folded

    @staticmethod
    def _normalize_values(values):
        total = sum(values[1:-1])
        return [v / total for v in values]

    def normalize_2d_sfs(self, sfs):
        """234-247: divide by sum(values[1:-1]) in insertion order."""
        self.sfs = sfs
        vals = self._normalize_values(list(sfs.values()))
        return dict(zip(sfs.keys(), vals))

    def normalize_1d_sfs(self, sfs):
        """465-476."""
        self.sfs = sfs
        vals = self._normalize_values(list(sfs.values()))
        return dict(zip(sfs.keys(), vals))

    def count_snps(self, window_data, variant_type):
        """291-302."""
        self.window_data = window_data
        self.variant_type = variant_type
        if variant_type is None:
            return len(window_data)
        return sum(1 for d in window_data.values() if d.get("annotation") == variant_type)

    def new_term(self, T1D, T2D):
        """779-785."""
        self.T1D = T1D
        self.T2D = T2D
        return T2D - T1D

    # dense-dict likelihoods: evaluated by the same GPU kernel on a synthetic SNP stream that
    # reproduces the given foreground spectrum (one SNP per count, no fold)
    def calculate_likelihood_2D(self, foreground_2d_sfs, background_2d_sfs):
        """625-684."""
        self.foreground_2d_sfs = foreground_2d_sfs
        self.background_2d_sfs = background_2d_sfs
        from sfs2d.dense import clr_2d
        return clr_2d(self._engine(), foreground_2d_sfs, background_2d_sfs, guards=True)

    def calculate_likelihood_1D(self, foreground_sfs, background_sfs):
        """478-537."""
        self.foreground_sfs = foreground_sfs
        self.background_sfs = background_sfs
        from sfs2d.dense import clr_1d
        return clr_1d(self._engine(), foreground_sfs, background_sfs, guards=True)

    # ------------------------------------------------------------------ helpers
    def _bg2d_array(self, bg):
        n1, n2 = 2 * self.pop1_size, 2 * self.pop2_size
        out = np.zeros((n1 + 1) * (n2 + 1), np.float64)
        keys = [(i, j) for i in range(n1 + 1) for j in range(n2 + 1)]
        for k, key in enumerate(keys[1:-1], start=1):
            out[k] = bg[key]            # background_2d_sfs[k] for k in bins[1:-1] (:658-661)
        return out

    @staticmethod
    def _bg1d_array(bg, pop_size):
        out = np.zeros(pop_size + 1, np.float64)
        for k in range(1, pop_size):
            out[k] = bg[k]              # background_sfs[k] for k in bins[1:-1] (:505-508)
        return out
