"""Test-only: a scan split over ranks at window boundaries (sfs2d.dist.scan_records_split) driven in ONE process.
K jobs on one engine stand in for K ranks, a sum over the buffer's first axis for the all-reduce: no
torch.distributed, no subprocess.  The jobs are dist_worker.FakeSplitJob (the oracle; host rows, no GPU) or
GpuSplitJob below (engine.SplitJob's calls on a plan that stays open, so that its rows can be read and it can run
again).  The fixtures, configs and cut lists of test_split_cpu.py / test_split_gpu.py are built here, by rule."""
import contextlib
import dataclasses

import numpy as np

import dist_worker as DW
from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import dist as D

LENGTHS = [6000, 2500, 700]
SEED = 5
VT = 1   # ann_want of the filtered variants: "intron_variant" of synth_genome(n_ann=3)
_DATA, _FAKE = {}, {}


# ----------------------------------------------------------------------------------------------------- fixtures

def genome(n1p, n2p, kind="plain"):
    """synth_genome(3, [6000, 2500, 700], n1p, n2p, seed 5) with three annotation classes.  kind "corner_part":
    every SNP of the second half of chromosome 1 (part 2 of the four-part cuts) lies in one of the two 2D bins
    bins[1:-1] leaves out of an unfolded spectrum -- alternately (0, 0) and (n1, n2) -- so that part's own inner
    2D and 1D sums are 0; "zero_chrom": every SNP of chromosome 1 does."""
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_genome
    key = (n1p, n2p, kind)
    if key in _DATA:
        return _DATA[key]
    p = synth_genome(3, LENGTHS, n1p, n2p, seed=SEED, n_ann=3)
    if kind != "plain":
        lo, hi = int(p.chrom_off[1]), int(p.chrom_off[2])
        if kind == "corner_part":
            lo = four_cuts(p, bp_cfg(n1p, n2p))[2]
        else:
            assert kind == "zero_chrom"
        i = np.arange(hi - lo)
        a1, a2 = np.where(i % 2 == 0, 0, 2 * n1p), np.where(i % 2 == 0, 0, 2 * n2p)
        counts = p.counts.copy()
        counts[lo:hi] = pack_counts(2 * n1p - a1, a1, 2 * n2p - a2, a2)
        p = PackedSNPs(counts, p.pos, p.chrom_off, list(p.chrom_names), p.ann_id, list(p.ann_names), p.pop1, p.pop2)
    _DATA[key] = p
    return p


def bp_cfg(n1p, n2p, window=20000, **kw):
    """Fixed-bp windows with the Q9 helper (the combined_scan plan)."""
    from sfs2d.engine import ScanConfig
    kw.setdefault("prev_extra", True)
    return ScanConfig(n1p=n1p, n2p=n2p, window=window, **kw)


def snp_cfg(n1p, n2p, window=500, **kw):
    from sfs2d.engine import ScanConfig
    return ScanConfig(n1p=n1p, n2p=n2p, window_mode=L.WINDOW_SNPS, window=window, **kw)


def four_cuts(p, cfg):
    """[0, a, b, c, n]: a the window start nearest one third of chromosome 0, b the one nearest the middle of
    chromosome 1 (both strictly inside their chromosome), c the chromosome 1 / 2 boundary."""
    st = D.window_starts(p, cfg)
    off = [int(x) for x in p.chrom_off]

    def nearest(t, lo, hi):
        s = st[(st > lo) & (st < hi)]
        assert len(s), "no window start strictly inside the chromosome: lengthen it"
        return int(s[np.argmin(np.abs(s - t))])

    a = nearest(off[0] + (off[1] - off[0]) / 3, off[0], off[1])
    b = nearest((off[1] + off[2]) / 2, off[1], off[2])
    return [0, a, b, off[2], off[3]]


def cut_lists(p, cfg):
    """{"four": the four-part cuts, "empty": the same with the middle cut repeated (part 2 holds no SNP)}."""
    c = four_cuts(p, cfg)
    return {"four": c, "empty": c[:3] + c[2:]}


def windows(p, cfg):
    """The oracle's windows of ``cfg`` over ``p`` in scan order (chrom, ..., begin, end)."""
    return O.bp_windows(p, int(cfg.window)) if cfg.window_mode == L.WINDOW_BP else O.snp_windows(p, int(cfg.window))[0]


def ocfg_of(p, cfg):
    return DW._fake_ocfg(p, cfg)


def backgrounds_of_rows(cfg, rows):
    """bg_of(c) -> (2D, folded 1D, folded 1D) from exchange rows [nchrom, >= W] (FakeSplitJob.finish's reading)."""
    n1, n2 = 2 * cfg.n1p, 2 * cfg.n2p
    nb = (n1 + 1) * (n2 + 1)
    bgs = [(t[:nb].reshape(n1 + 1, n2 + 1), O.fold1d(t[nb:nb + n1 + 1]), O.fold1d(t[nb + n1 + 1:nb + n1 + n2 + 2]))
           for t in np.asarray(rows, np.int64)]
    return lambda c: bgs[c]


def strip(t):
    """dist_worker._strip: empty slots dropped, the Q9 helper's wid zeroed."""
    return DW._strip(np.asarray(t, dtype=L.WINDOW_DTYPE))


# -------------------------------------------------------------------------------------------------------- jobs

class GpuSplitJob:
    """One part on the GPU: its SNPs resident (uploaded, or handed over as device arrays: ``wrap``), one plan (and
    one plan attached to it: ``attach``).  The calls are engine.SplitJob's, but nothing is closed by them."""

    def __init__(self, eng, sub, cfg, bg=None, wrap=False, attach=None):
        import wide_util
        self.eng, self.sub, self.cfg = eng, sub, cfg
        self.keep = self.pl = self.att = None
        if wrap:
            self.dev, self.keep = wide_util.wrapped(eng, sub, ann=cfg.ann_want >= 0)
        else:
            self.dev = eng.upload(sub)
        try:
            self.pl = eng.plan(self.dev, cfg)
            if cfg.bg_mode == L.BG_SUPPLIED:
                self.pl.set_background(*bg)
            if attach is not None:
                self.att = self.pl.attach(attach)
        except Exception:
            self.close()
            raise

    def whole(self):
        """An ordinary run of the part on its own: (records, Fst or None)."""
        self.pl.run()
        self.pl.check()
        return self.pl.read(), self.fst()

    def partial_dev(self, rows_ptr, stride):
        self.pl.run(phase=1)
        self.rows_get(rows_ptr, stride)

    def rows_get(self, rows_ptr, stride):
        import ctypes as C
        self.eng.check(self.eng.lib.sfs2d_plan_bg_rows_dev(self.pl.h, C.c_void_p(rows_ptr), int(stride)))

    def rows_set(self, rows_ptr, stride):
        import ctypes as C
        self.eng.check(self.eng.lib.sfs2d_plan_bg_rows_set_dev(self.pl.h, C.c_void_p(rows_ptr), int(stride)))

    def phase2(self):
        self.pl.run(phase=2)
        self.pl.check()
        return self.pl.read()

    def finish_dev(self, rows_ptr, stride):
        if self.cfg.bg_mode != L.BG_PER_CHROM:
            return self.whole()[0]
        self.rows_set(rows_ptr, stride)
        return self.phase2()

    def fst(self):
        return self.pl.read_fst() if self.cfg.fst else None

    def attached(self):
        """(records, Fst or None) of the attached plan after the base's run."""
        return self.att.read(), (self.att.read_fst() if self.att.cfg.fst else None)

    def close(self):
        if self.pl is not None:
            self.pl.close()
            self.pl = self.att = None
        if self.dev is not None:
            self.dev.close()
            self.dev = None
        self.keep = None


class GpuJobs:
    """make_job of split_in_process for GpuSplitJob parts on ``eng``."""

    def __init__(self, eng, wrap=False, attach=None):
        self.eng, self.wrap, self.attach = eng, wrap, attach

    def __call__(self, sub, cfg, bg):
        return GpuSplitJob(self.eng, sub, cfg, bg, wrap=self.wrap, attach=self.attach)


class Reuse:
    """make_job that hands out the jobs of an earlier split again, in order (a second split on the same plans)."""

    def __init__(self, res):
        self.jobs = [j for j in res.jobs if j is not None]
        self.eng = getattr(self.jobs[0], "eng", None) if self.jobs else None

    def __call__(self, sub, cfg, bg):
        return self.jobs.pop(0)


@contextlib.contextmanager
def on_stream(eng):
    """The library's kernels and torch's ops ordered on one fresh stream (sfs2d.dist._one_stream); the engine's
    previous stream is restored on exit (Engine.get(0) is shared by the whole suite)."""
    import torch
    with D._one_stream(eng, torch.device(f"cuda:{eng.device}")) as s:
        yield s


@dataclasses.dataclass
class SplitResult:
    table: np.ndarray     # the merged table (sfs2d.dist._merge_split)
    tables: list          # each part's records as its plan numbers them (empty parts: 0 records)
    rows: list            # each part's rows [its chromosomes, stride] after phase 1 (None: empty part)
    buffer: np.ndarray    # the whole exchange buffer [K, nchrom, stride] after every part's rows were written
    total: np.ndarray     # the summed rows [nchrom, stride]
    fst: list             # each part's Fst column per slot (None: no Fst / empty part / oracle job)
    jobs: list            # the parts' jobs, still open (None: empty part)
    cuts: list
    c0s: list             # each part's first chromosome
    subs: list            # each part's data set

    def close(self):
        for j in self.jobs:
            if j is not None:
                j.close()

    def merged_fst(self):
        """The Fst of the merged table's windows, in its order (None without Fst)."""
        out = []
        for t, f in zip(self.tables, self.fst):
            if f is None:
                continue
            out.append(f[(t["flags"][: len(f)] & L.W_EMPTY) == 0])
        return np.concatenate(out) if out else None


def split_in_process(p, cfg, cuts, make_job, bg=None, stride=None, prior_runs=0):
    """scan_records_split's steps for the parts [cuts[r], cuts[r+1]) of ``p``, in this process.  Every part's
    phase 1 writes its rows into its slice of ONE int64 buffer [K, nchrom, stride] (zero, the padding words of a
    stride above the row width -1), the sum over K is every chromosome's total, and every part finishes from the
    rows of its chromosomes.  ``prior_runs``: ordinary runs of every part's plan first."""
    K = len(cuts) - 1
    W = D.hist_width(cfg)
    stride = W if stride is None else int(stride)
    parts = [p.slice_snps(cuts[r], cuts[r + 1]) for r in range(K)]
    subs, c0s = [s for s, _ in parts], [c for _, c in parts]
    live = [r for r in range(K) if cuts[r + 1] > cuts[r]]
    last = live[-1] if live else -1   # the Q9 helper: the last non-empty part's, as scan_records_split
    eng = getattr(make_job, "eng", None)
    jobs, rows, fst = [None] * K, [None] * K, [None] * K
    tables = [np.zeros(0, dtype=L.WINDOW_DTYPE) for _ in range(K)]
    with (on_stream(eng) if eng is not None else contextlib.nullcontext()):
        try:
            for r in live:
                jobs[r] = make_job(subs[r], dataclasses.replace(cfg, prev_extra=bool(cfg.prev_extra) and r == last), bg)
            if eng is None:
                buf = np.zeros((K, p.nchrom, stride), np.int64)
            else:
                import torch
                buf = torch.zeros((K, p.nchrom, stride), dtype=torch.int64, device=f"cuda:{eng.device}")
            buf[:, :, W:] = -1
            for r in live:
                for _ in range(prior_runs):
                    jobs[r].whole()
                if not W:
                    continue
                if eng is None:
                    buf[r, c0s[r]:c0s[r] + subs[r].nchrom, :W] = jobs[r].partial()
                else:
                    jobs[r].partial_dev(buf[r, c0s[r]].data_ptr(), stride)
            total = buf.sum(0)   # the all-reduce
            hbuf = buf.copy() if eng is None else buf.cpu().numpy()
            htot = total.copy() if eng is None else total.cpu().numpy()
            for r in live:
                a, b = c0s[r], c0s[r] + subs[r].nchrom
                rows[r] = hbuf[r, a:b].copy()
                if eng is None:
                    tables[r] = jobs[r].finish(total[a:b, :W] if W else None)
                else:
                    tables[r] = jobs[r].finish_dev(total[a].data_ptr() if W else None, stride)
                    fst[r] = jobs[r].fst()
        except Exception:
            for j in jobs:
                if j is not None:
                    j.close()
            raise
    table = D._merge_split(tables, cuts, c0s, bool(cfg.prev_extra),
                           int(cfg.window) if cfg.window_mode == L.WINDOW_SNPS else 0, p.chrom_off)
    return SplitResult(table, tables, rows, hbuf, htot, fst, jobs, list(cuts), c0s, subs)


def fake_split(key, p, cfg, cuts, stride=None):
    """split_in_process with the oracle's jobs, computed once per ``key`` and shared."""
    if key not in _FAKE:
        _FAKE[key] = split_in_process(p, cfg, cuts, DW.FakeSplitJob, stride=stride)
    return _FAKE[key]


# ------------------------------------------------------------------------------------------------------- cases
# What the GPU tests run, by name: (grid, data kind, ScanConfig).  test_split_cpu.py runs every one of them through
# the driver with the oracle's jobs, over both cut lists.

GRIDS_ROWS = [(25, 25), (10, 30), (60, 35)]
GRIDS_LARGE = [(50, 50), (60, 35)]


def filter_positions(p):
    """start_position / end_position of the filtered variants: they cut into chromosome 0 and chromosome 1 on
    both sides and leave chromosome 2 (shorter than the start) without a SNP in the SFS."""
    return int(p.pos[int(p.chrom_off[3]) - 1]) + 1, int(p.pos[int(p.chrom_off[1]) + 2000])


def row_variants(n1p, n2p):
    p = genome(n1p, n2p)
    s, e = filter_positions(p)
    return {"fold": bp_cfg(n1p, n2p), "nofold": bp_cfg(n1p, n2p, fold=False),
            "ann": snp_cfg(n1p, n2p, ann_want=VT), "pos": bp_cfg(n1p, n2p, fold=False, start_position=s, end_position=e)}


def w_cfgs(fst):
    """The k_scan_w rows of the matrix: 20 kb with the Q9 helper, and 500-SNP windows."""
    return {"bp20k": bp_cfg(25, 25, fst=fst), "snp500": snp_cfg(25, 25, fst=fst)}


def hist_cfg(n1p, n2p):
    """(h) every filter at once: unfolded, variant_type and both position bounds."""
    s, e = filter_positions(genome(n1p, n2p))
    return bp_cfg(n1p, n2p, fold=False, ann_want=VT, start_position=s, end_position=e)


def end_filter_cfg(n1p=25, n2p=25):
    """(e) end_position at the last SNP before the middle cut of chromosome 1: no SNP of part 2 enters the SFS."""
    p = genome(n1p, n2p)
    b = four_cuts(p, bp_cfg(n1p, n2p))[2]
    return bp_cfg(n1p, n2p, fst=True, end_position=int(p.pos[b - 1]))


def all_cases():
    """{name: (p, cfg)} of every (data set, config) a GPU test splits."""
    out = {}
    for n1p, n2p in GRIDS_ROWS:
        for v, cfg in row_variants(n1p, n2p).items():
            out[f"rows-{n1p}x{n2p}-{v}"] = (genome(n1p, n2p), cfg)
    for fst in (False, True):
        for w, cfg in w_cfgs(fst).items():
            out[f"w-{w}-fst{int(fst)}"] = (genome(25, 25), cfg)
    for n1p, n2p in GRIDS_LARGE:
        out[f"large-{n1p}x{n2p}"] = (genome(n1p, n2p), bp_cfg(n1p, n2p, fst=True))
    for n1p, n2p in GRIDS_ROWS[1:]:
        out[f"hist-{n1p}x{n2p}"] = (genome(n1p, n2p), hist_cfg(n1p, n2p))
    out["wide-70k"] = (genome(25, 25), bp_cfg(25, 25, window=70000, fold=False, prev_extra=False, fst=True))
    out["attach-100k"] = (genome(25, 25), bp_cfg(25, 25, window=100000, prev_extra=False, fst=True))
    out["corner_part"] = (genome(25, 25, "corner_part"), bp_cfg(25, 25, fold=False, fst=True))
    out["zero_chrom"] = (genome(25, 25, "zero_chrom"), bp_cfg(25, 25, fold=False, fst=True))
    out["end_filter"] = (genome(25, 25), end_filter_cfg())
    return out
