"""k_scan_w's variants against the oracle, window by window: the plan bench.py times (Fst in the scan, one
scan workgroup per CU, passes overlapped on two streams), the D table's last entry (ranks 510 .. 1024 in
one bin), data that must take the ungated variant (over-called SNPs, unfolded spectra) and Fst's edge
values.  Counts exact, T2D / T1D by golden_util.close, Fst within 1e-12 + 1e-10 |x| of O.window_fst."""
import numpy as np
import pytest

import golden_util as gu
from oracle import sfs_oracle as O
from wide_util import check_records as _check

pytestmark = pytest.mark.gpu

POP, WS = 25, 20000


def _bench_genome():
    from sfs2d.synth import synth_genome
    return synth_genome(3, [40000, 12000, 700], POP, POP, seed=4242)


_REF = {}


def _oracle(key, p, fold=True):
    """(windows, records, Fst) of every non-empty 20 kb window, per-chromosome backgrounds; computed once
    per data set and shared."""
    if key not in _REF:
        ocfg = O.Cfg(POP, POP, fold=fold)
        bgs = O.chrom_backgrounds(p, ocfg)
        wins = O.bp_windows(p, WS)
        recs = O.window_records(p, wins, ocfg, lambda c: bgs[c])
        fst = [O.window_fst(p, np.arange(w[2], w[3]), ocfg) for w in wins]
        _REF[key] = (wins, recs, fst)
    return _REF[key]


def _scan(p, **kw):
    """One plan run: (records, Fst)."""
    from sfs2d.engine import Engine, ScanConfig
    eng = Engine.get(0)
    dev = eng.upload(p)
    pl = eng.plan(dev, ScanConfig(n1p=POP, n2p=POP, window=WS, fst=True, **kw))
    pl.run()
    pl.check()
    out = pl.read(), pl.read_fst()
    pl.close()
    dev.close()
    return out


def test_benchmarked_plan_vs_oracle():
    """bench.py's config-3 plan at a small size: two plans of ScanConfig(window=20000, fst=True,
    scan_wgs_per_cu=1), 4 passes round-robin on 2 streams; both tables byte-equal, every window the oracle's."""
    import torch
    from sfs2d import _lib as L
    from sfs2d.engine import Engine, Plan, ScanConfig
    p = _bench_genome()
    eng = Engine.get(0)
    dev = eng.upload(p)
    cfg = ScanConfig(n1p=POP, n2p=POP, window=WS, fst=True, scan_wgs_per_cu=1)
    plans = [eng.plan(dev, cfg) for _ in range(2)]
    assert plans[0].scan_kernel() == "k_scan_w"
    streams = [torch.cuda.Stream(device=0).cuda_stream for _ in range(2)]
    outs = [torch.zeros((plans[0].nrec, 64), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    Plan.run_streams(plans, streams, 4, [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    for q in plans:
        q.check()
    tabs = [o.cpu().numpy().tobytes() for o in outs]
    assert tabs[0] == tabs[1]
    fsts = [q.read_fst() for q in plans]
    assert fsts[0].tobytes() == fsts[1].tobytes()
    _check(np.frombuffer(tabs[0], dtype=L.WINDOW_DTYPE), fsts[0], _oracle("bench", p))
    for q in plans:
        q.close()
    dev.close()


def _one_bin_chrom():
    """One chromosome of 20 kb windows: mixed SNPs | 511 | (empty slot) | 512 | 513 | monomorphic | 1025 | mixed,
    the sized windows each of one in-grid counts word (one 2D bin: ranks up to 510, 511, 512 and 1024)."""
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(11))
    _, r1, a1, r2, a2 = synth_chrom(rng, 500, POP, POP)
    mixed = pack_counts(r1, a1, r2, a2)
    word = lambda x1, x2: int(pack_counts(np.array([50 - x1]), np.array([x1]), np.array([50 - x2]), np.array([x2]))[0])
    layout = [(0, mixed[:300]), (1, np.full(511, word(3, 7))), (3, np.full(512, word(10, 2))),
              (4, np.full(513, word(1, 1))), (5, np.full(100, word(0, 0))), (6, np.full(1025, word(20, 24))),
              (7, mixed[300:])]
    counts, pos = [], []
    for w, c in layout:
        n = len(c)
        counts.append(np.asarray(c, np.uint32))
        pos.append(w * WS + 1 + np.arange(n, dtype=np.int64) * (19000 // n))
    counts, pos = np.concatenate(counts), np.concatenate(pos).astype(np.uint32)
    return PackedSNPs(counts, pos, np.array([0, len(counts)], np.int64), ["chr0000"], np.zeros(len(counts), np.uint16),
                      ["intergenic_region"], "p1", "p2")


def test_d_table_boundary_ranks():
    """Windows of exactly 511, 512, 513 and 1025 SNPs in one bin: the first 8 rows' ranks reach LNT-1 = 511
    without a clamp, the streamed rows pass the table (its correction pass), a monomorphic window and an
    empty slot in between."""
    p = _one_bin_chrom()
    ref = _oracle("onebin", p)
    assert [w[3] - w[2] for w in ref[0]] == [300, 511, 512, 513, 100, 1025, 200]
    assert ref[1][4]["N2"] == 0 and ref[1][5]["N2"] == 1025
    for cap in (0, 1):
        recs, fst = _scan(p, scan_wgs_per_cu=cap)
        assert len(recs) == 8   # slot 2 is empty
        _check(recs, fst, ref)


def _overcalled_genome():
    """The benchmarked data with a handful of SNPs whose r + a exceeds 2 pop_size (keys inside the grid),
    one of them with the folded key (n1, n2), the excluded last bin."""
    from sfs2d.pack import PackedSNPs, pack_counts
    p = _bench_genome()
    counts = p.counts.copy()
    pc = lambda r1, a1, r2, a2: int(pack_counts(np.array([r1]), np.array([a1]), np.array([r2]), np.array([a2]))[0])
    counts[5] = pc(50, 26, 50, 25)        # a1 + a2 > 50: folds to (r1, r2) = (50, 50), the last bin
    counts[777] = pc(40, 20, 30, 10)      # over-called in population 1, unfolded key (20, 10)
    counts[20000] = pc(30, 45, 20, 40)    # folds to (30, 20); over-called in both
    counts[41000] = pc(49, 3, 50, 1)      # second chromosome
    counts[52500] = pc(10, 50, 12, 45)    # third chromosome: alt count at the grid's edge
    return PackedSNPs(counts, p.pos, p.chrom_off, list(p.chrom_names), p.ann_id, list(p.ann_names), p.pop1, p.pop2)


@pytest.mark.parametrize("fold", [True, False])
def test_overcalled_and_unfolded_take_the_ungated_variant(fold):
    """Over-called counts (max_nc > 2 pop_size at upload) and unfolded plans keep the scan's range test: the
    SNP in the excluded last bin stays out of n2 and is counted in n2_all, and every window matches the
    oracle, n2_all included: a folded plan's scan counts the last bin's SNPs whenever the data is
    over-called (only such data can fold a SNP to (n1, n2))."""
    p = _overcalled_genome()
    ref = _oracle(("over", fold), p, fold=fold)
    if fold:
        assert ref[1][0]["N2_all"] == ref[1][0]["N2"] + 1   # the (n1, n2) SNP sits in the first window
    recs, fst = _scan(p, fold=fold, scan_wgs_per_cu=1)
    _check(recs, fst, ref)
    if fold:
        assert int(recs[0]["n2_all"]) == int(recs[0]["n2"]) + 1


def _last_bin_window_genome(n1p, n2p, S):
    """Two chromosomes of ordinary SNPs; SNP S + 1 (inside the second S-SNP window of the first) is
    over-called so that it folds to (n1, n2), the excluded last bin: (2 n1p, n1p + 1, 2 n2p, n2p)."""
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_genome
    p = synth_genome(2, [5 * S + 3, 2 * S], n1p, n2p, seed=31 + n1p)
    counts = p.counts.copy()
    counts[S + 1] = int(pack_counts(np.array([2 * n1p]), np.array([n1p + 1]), np.array([2 * n2p]), np.array([n2p]))[0])
    return PackedSNPs(counts, p.pos, p.chrom_off, list(p.chrom_names), p.ann_id, list(p.ann_names), p.pop1, p.pop2)


@pytest.mark.parametrize("n1p,n2p,kernel", [(25, 25, "k_scan_w"), (50, 50, "k_scan_gw")])
def test_last_bin_snp_counts_in_n2_all(n1p, n2p, kernel):
    """A folded plan's S-SNP window holding one SNP of the excluded last bin among ordinary SNPs:
    n2_all == n2 + 1 exactly in both fast scans (the rule scan_*_bySNPs skips windows by), every record's
    integers as the oracle's."""
    from sfs2d import _lib as L
    from sfs2d.engine import Engine, ScanConfig
    S = 70
    p = _last_bin_window_genome(n1p, n2p, S)
    ocfg = O.Cfg(n1p, n2p)
    bgs = O.chrom_backgrounds(p, ocfg)
    wins = O.snp_windows(p, S)[0]
    orec = O.window_records(p, wins, ocfg, lambda c: bgs[c])
    assert orec[1]["N2_all"] == orec[1]["N2"] + 1 and orec[1]["N2"] > 0
    assert all(o["N2_all"] == o["N2"] for i, o in enumerate(orec) if i != 1)
    eng = Engine.get(0)
    dev = eng.upload(p)
    pl = eng.plan(dev, ScanConfig(n1p=n1p, n2p=n2p, window_mode=L.WINDOW_SNPS, window=S))
    assert pl.scan_kernel() == kernel
    pl.run()
    pl.check()
    recs = pl.read()
    pl.close()
    dev.close()
    assert len(recs) == len(wins)
    for i, (w, r, o) in enumerate(zip(wins, recs, orec)):
        assert (int(r["chrom"]), int(r["begin"]), int(r["end"])) == (w[0], w[-2], w[-1]), (i, w)
        for a, b in (("snp_count", "snp_count"), ("n2", "N2"), ("n2_all", "N2_all"), ("n1a", "N1a"), ("n1b", "N1b")):
            assert int(r[a]) == o[b], (i, a, int(r[a]), o[b])
        for a, b in (("t2d", "T2D"), ("t1d_p1", "T1D_p1"), ("t1d_p2", "T1D_p2")):
            assert o[b] is not None and gu.close(float(r[a]), o[b]), (i, a, float(r[a]), o[b])
    assert int(recs[1]["n2_all"]) == int(recs[1]["n2"]) + 1


def _bysnp_chrom(last_bin):
    """One chromosome of 40 polymorphic SNPs at pop 25 / 25, scanned in windows of S = 4; window 5 holds
    monomorphic SNPs (50, 0, 50, 0) and, with last_bin, the over-called SNP (50, 26, 50, 25), which folds
    to (n1, n2): the window's 2D SFS then holds one SNP, in the bin bins[1:-1] leaves out."""
    from sfs2d.pack import PackedSNPs, pack_counts
    i = np.arange(40)
    a1, a2 = 1 + (7 * i) % 48, 1 + (11 * i) % 48
    r1, r2 = 50 - a1, 50 - a2
    a1[20:24], a2[20:24], r1[20:24], r2[20:24] = 0, 0, 50, 50
    if last_bin:
        r1[21], a1[21], r2[21], a2[21] = 50, 26, 50, 25
    return PackedSNPs(pack_counts(r1, a1, r2, a2), (100 + 37 * i).astype(np.uint32), np.array([0, 40], np.int64),
                      ["chr0000"], np.zeros(40, np.uint16), ["intergenic_region"], "p1", "p2")


def test_bysnps_enters_a_window_of_one_last_bin_snp():
    """scan_perChr_bySNPs skips a window whose 2D SFS is empty (n2_all == 0).  A window holding only
    monomorphic SNPs and one SNP of the last bin is entered: T2D is None there and the reference's
    T2D - T1D_pop1 raises TypeError, as the oracle's."""
    import twoDSFS_class as T
    p = _bysnp_chrom(True)
    with pytest.raises(TypeError):
        O.scan_perChr_bySNPs(p, 4, O.Cfg(POP, POP))
    obj = T.LikelihoodInference_jointSFS(None, None, pop1="p1", pop2="p2", pop1_size=POP, pop2_size=POP)
    with pytest.raises(TypeError):
        obj.scan_perChr_bySNPs(p, 4)


def test_bysnps_skips_a_monomorphic_window():
    """The same chromosome with window 5 all monomorphic: skipped, the other 9 windows are the oracle's."""
    import twoDSFS_class as T
    p = _bysnp_chrom(False)
    want = O.scan_perChr_bySNPs(p, 4, O.Cfg(POP, POP))
    assert len(want) == 9
    obj = T.LikelihoodInference_jointSFS(None, None, pop1="p1", pop2="p2", pop1_size=POP, pop2_size=POP)
    assert gu.compare_results(obj.scan_perChr_bySNPs(p, 4), want) == []


def _fst_edge_chrom(low_nc):
    """Mixed SNPs with a = 0, a = 1 and a = n in either population written over some of them; low_nc: SNPs with
    fewer than 2 called alleles in one population as well (the masked variant), one window of them alone."""
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(23))
    pos, r1, a1, r2, a2 = synth_chrom(rng, 3000, POP, POP)
    edge = [(50, 0, 49, 1), (49, 1, 50, 0), (0, 50, 25, 25), (25, 25, 0, 50), (0, 50, 49, 1), (49, 1, 0, 50),
            (50, 0, 0, 50), (0, 50, 50, 0), (1, 1, 25, 25), (0, 2, 30, 20), (2, 0, 1, 1)]
    if low_nc:
        edge += [(1, 0, 25, 25), (0, 1, 25, 25), (25, 25, 0, 1), (0, 0, 25, 25), (25, 25, 0, 0), (0, 1, 0, 1)]
    for k in range(600):
        r1[2 * k + 1], a1[2 * k + 1], r2[2 * k + 1], a2[2 * k + 1] = edge[k % len(edge)]
    if low_nc:   # the last window: no SNP with 2 called alleles in both populations (Fst NaN)
        last = (np.maximum(pos, 1) - 1) // WS == (pos[-1] - 1) // WS
        r1[last], a1[last] = 0, 1
    counts = pack_counts(r1, a1, r2, a2)
    return PackedSNPs(counts, pos.astype(np.uint32), np.array([0, len(counts)], np.int64), ["chr0000"],
                      np.zeros(len(counts), np.uint16), ["intergenic_region"], "p1", "p2")


@pytest.mark.parametrize("low_nc", [False, True])
def test_fst_edge_values(low_nc):
    """a = 0, 1 and n in either population (a (a - 1) = 0 exactly), and the masked variant's SNPs with fewer
    than 2 called alleles in a population, NaN windows included."""
    p = _fst_edge_chrom(low_nc)
    ref = _oracle(("fst", low_nc), p)
    if low_nc:
        assert ref[2][-1] is None
    recs, fst = _scan(p, scan_wgs_per_cu=1)
    _check(recs, fst, ref)
