"""Test-only: fixtures and shared pieces of the after-run tests (test_after_run_cpu.py, test_after_run_gpu.py).

The post-scan calls (sfs2d_plan_null_run / _null_run_blocks, _diversity, _spectra, _project) and sfs2d_plan_read /
_fst_read work on "the plan's last run".  A stale buffer shows only when the data changed between runs, so the
fixtures come in pairs: two data sets A and B with identical host-side facts (SNP count, chrom_off, chromosome and
annotation names, every chromosome's first and last position), so that ONE sfs2d_data_wrap_device data set can be
rewritten in place from A to B and back (``Wrapped.rewrite``), as its contract allows.

  A  ``pair("small")``: project_util.genome(18, 14, (24, 20)) -- chromosomes of 1 .. 9,000 SNPs, 14,057 in all, 2 %
     missing alleles, the projection's planted kinds, annotations -- with one more planted kind, ``last_inner``: an
     over-called SNP that the joint fold sends to (2 n1p, 2 n2p - 1), the last inner 2D bin, every 293rd SNP of the
     last chromosome.  The generated SNPs never reach that bin, and it is the one bin a background table without its
     tail (scipy's p[-1] rule, k_null_tail) gets wrong.
     ``pair("large")``: project_util.genome(50, 50, None, lengths=[2049, 1000, 257], full=True), 3,306 SNPs.
  B  ``derive(A)``: every chromosome's positions mirrored, pos_B[i] = pos_A[first] + pos_A[last] - pos_A[last - i]
     (strictly increasing like A's, first and last position kept), and the (counts, ann_id) pairs rotated cyclically
     over the whole data set by ``OFFSET`` SNPs (the multiset of SNPs, hence every planted kind, is kept; every
     chromosome's background changes).

``KINDS`` are the plan kinds the GPU tests run, by name; ``slot_records`` gives the oracle's record of every window
slot of a kind (computed once per (data, geometry, filters, background) and shared -- read-only), on which
test_after_run_cpu.py asserts that A and B differ enough for a stale read to show."""
import numpy as np

import project_util as PU
import wide_util as WU
from oracle import sfs_oracle as O
from sfs2d import _lib as L

OFFSET = 4001
N_SMALL, M_SMALL = (18, 14), (24, 20)
N_LARGE, M_LARGE = (50, 50), (50, 50)
BIG = [2049, 1000, 257]
FILT = {"start_position": 3000, "end_position": 400000, "ann_want": 1}     # test_project_gpu.FILT
NULL_REPS, NULL_SEED, NULL_BLOCK = 8, 3, 16
_PAIR, _SLOTS = {}, {}


def last_inner(n1p, n2p):
    """(ref1, alt1, ref2, alt2): alt1 + alt2 > n1p + n2p, so the fold takes the refs (2 n1p, 2 n2p - 1)."""
    return (2 * n1p, n1p + 1, 2 * n2p - 1, n2p)


def derive(a, offset=OFFSET):
    from sfs2d.pack import PackedSNPs
    pos = a.pos.astype(np.int64).copy()
    for c in range(a.nchrom):
        lo, hi = int(a.chrom_off[c]), int(a.chrom_off[c + 1])
        if hi > lo:
            pos[lo:hi] = pos[lo] + pos[hi - 1] - pos[lo:hi][::-1]
    return PackedSNPs(np.roll(a.counts, offset), pos, a.chrom_off.copy(), list(a.chrom_names), np.roll(a.ann_id, offset),
                      list(a.ann_names), a.pop1, a.pop2)


def pair(which):
    """(A, B) of ``which`` ("small" / "large"); built once, read-only."""
    if which not in _PAIR:
        from sfs2d.pack import PackedSNPs, pack_counts
        if which == "small":
            g = PU.genome(*N_SMALL, M_SMALL)
            counts = g.counts.copy()
            big = int(g.chrom_off[-2])
            planted = set(range(5, g.n, 41)) | {big + x for x in (0, 63, 64, 255, 256, 257, 1023, 1024, 1025)} | {g.n - 1}
            at = [i for i in range(big + 100, g.n, 293) if i not in planted]
            counts[at] = pack_counts(*[[v] * len(at) for v in last_inner(*N_SMALL)])
            a = PackedSNPs(counts, g.pos, g.chrom_off, list(g.chrom_names), g.ann_id, list(g.ann_names), g.pop1, g.pop2)
        else:
            a = PU.genome(*N_LARGE, None, lengths=BIG, full=True)
        b = derive(a)
        _PAIR[which] = (a, b)
    return _PAIR[which]


def tasks(which, supplied=False):
    """The null tasks of the tests: a single draw, one wave's worth, two rounds of pairs, and more draws than a lane
    keeps in registers, from a small and the largest chromosome (pool -1, every SNP, where one supplied table is
    every pool's background)."""
    t = [(0, 1), (7, 64), (9, 129), (9, 513)] if which == "small" else [(2, 1), (1, 64), (0, 129), (0, 513)]
    return t + ([(-1, 64)] if supplied else [])


# ---------------------------------------------------------------------------------------------------- plan kinds
# name -> which pair, environment, ScanConfig arguments (pop sizes aside), projection, what scan_kernel() /
# scan_variant() must report (the sliding plan keeps 16-bit bins on wrapped data too: positions are strictly increasing by
# the data set's contract, so a window of 8,000 bp holds at most 8,000 SNPs; test_wide_bins.py's 32-bit sliding plans
# are the ones above 65,535 bp), and the extras: ann (the wrapped data carries annotation ids), supplied (one background
# table: chromosome SUPPLIED_CHROM of A's, kept whatever the data), attach (ScanConfig arguments of a plan attached
# to this base: the record calls go to it, the null to the base).
SUPPLIED_CHROM = 9
KINDS = {
    "fused": dict(env={"SFS2D_FUSED": "1"}, cfg=dict(window=20000, fst=True), kernel="k_scan_w", variant={"fused": 1, "cnt": 1}),
    "sliced": dict(env={"SFS2D_FUSED": "0"}, cfg=dict(window=20000, fst=True), kernel="k_scan_w", variant={"fused": 0, "cnt": 1}),
    "gw": dict(which="large", env={"SFS2D_GW": "1"}, cfg=dict(window=20000, fst=True), kernel="k_scan_gw", variant={}),
    "filtered": dict(cfg=dict(window=20000, fst=True, **FILT), ann=True, kernel="k_scan_w", variant={"cnt": 0}),
    "snp257": dict(cfg=dict(window_mode=L.WINDOW_SNPS, window=257, fst=True), kernel="k_scan_w", variant={"cnt": 1}),
    "sliding": dict(cfg=dict(window=8000, step=2000, fst=True), kernel="k_scan_w", variant={"p16": 1}),
    "supplied": dict(cfg=dict(window=20000, fst=True, bg_mode=L.BG_SUPPLIED), supplied=True, kernel="k_scan_w", variant={}),
    "prev_extra": dict(cfg=dict(window=20000, fst=True, prev_extra=True), kernel="k_scan_w", variant={"cnt": 1}),
    "attached": dict(cfg=dict(window=2000, fst=True), attach=dict(window=10000, fst=True), kernel="k_scan_w", variant={}),
}
EVERY_ROUTE = ("fused", "sliced", "gw")


def which_of(kind):
    return KINDS[kind].get("which", "small")


def sizes(kind):
    """((n1p, n2p), (m1, m2)) of a kind."""
    return (N_LARGE, M_LARGE) if which_of(kind) == "large" else (N_SMALL, M_SMALL)


def scan_config(kind, attached=False):
    from sfs2d.engine import ScanConfig
    n1p, n2p = sizes(kind)[0]
    return ScanConfig(n1p=n1p, n2p=n2p, **(KINDS[kind]["attach"] if attached else KINDS[kind]["cfg"]))


def record_config(kind):
    """The ScanConfig whose records the record calls (read, diversity, spectra, project) see."""
    return scan_config(kind, attached="attach" in KINDS[kind])


def oracle_cfg(cfg, p):
    vt = None if cfg.ann_want < 0 else p.ann_names[cfg.ann_want]
    return O.Cfg(cfg.n1p, cfg.n2p, vt, cfg.fold, cfg.start_position, cfg.end_position)


def supplied_background(kind):
    """(2D, folded 1D, folded 1D) of chromosome SUPPLIED_CHROM of the kind's A, under the kind's filters."""
    a = pair(which_of(kind))[0]
    return O.chrom_backgrounds(a, oracle_cfg(scan_config(kind), a))[SUPPLIED_CHROM]


def background_of(kind, p):
    """bg_of(chrom) of a kind's plans over data set ``p`` (the base's and the attached plan's alike)."""
    if KINDS[kind].get("supplied"):
        one = supplied_background(kind)
        return lambda c: one
    bgs = O.chrom_backgrounds(p, oracle_cfg(scan_config(kind), p))
    return lambda c: bgs[c]


# ---------------------------------------------------------------------------------------------------- slot records

def slot_windows(p, cfg):
    """Every window slot of ``cfg`` over ``p`` in record order: [(chrom, wid, begin, end)], begin == end: empty."""
    if cfg.window_mode == L.WINDOW_SNPS:
        return [(c, k, b, e) for k, (c, _, _, b, e) in enumerate(O.snp_windows(p, int(cfg.window))[0])]
    w = int(cfg.window)
    return WU.sliding_slots(p, w, int(cfg.step) if cfg.step else w)


def slot_records(kind, p):
    """(slots, oracle record or None per slot) of the kind's record plan over ``p``; shared, read-only."""
    cfg = record_config(kind)
    key = (id(p), kind if KINDS[kind].get("supplied") else None, cfg.window_mode, int(cfg.window), cfg.step, cfg.ann_want,
           cfg.start_position, cfg.end_position)
    if key not in _SLOTS:
        slots = slot_windows(p, cfg)
        live = [s for s in slots if s[3] > s[2]]
        recs = iter(O.window_records(p, live, oracle_cfg(cfg, p), background_of(kind, p)))
        _SLOTS[key] = (slots, [next(recs) if s[3] > s[2] else None for s in slots])
    return _SLOTS[key]


# ---------------------------------------------------------------------------------------------------- on the device

class Wrapped:
    """One sfs2d_data_wrap_device data set holding ``p``, rewritten in place by ``rewrite`` (the arrays are the
    caller's and may be written between runs; every host-side fact of the pair is the same)."""

    def __init__(self, eng, p, ann=False):
        self.eng, self.ann = eng, ann
        self.dev, self.keep = WU.wrapped(eng, p, ann=ann)
        self.now = p

    def rewrite(self, p):
        import torch
        torch.cuda.synchronize()          # nothing of the library's still reads the arrays
        counts, pos, annt = self.keep
        counts[: p.n].copy_(torch.from_numpy(p.counts.view(np.int32)))
        pos[: p.n].copy_(torch.from_numpy(p.pos.view(np.int32)))
        if self.ann:
            annt[: p.n].copy_(torch.from_numpy(p.ann_id.view(np.int16)))
        torch.cuda.synchronize()          # the library reads them on its own stream
        self.now = p

    def close(self):
        self.dev.close()
        self.keep = None
