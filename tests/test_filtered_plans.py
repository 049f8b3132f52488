"""The bins pipeline against the oracle: plans with a position or variant_type filter.  k_prep<DO_BINS, FILT>
(with and without its own fixed-point Fst sums) writes a 4-byte bins word per SNP, and the scans' non-CNT
instantiations (k_scan_w, k_scan_gw, k_scan_g), eval_exact, k_fst_win and k_bg_slice's Fst workgroups read
those words.  Every case compares a filtered plan's records with O.window_records and O.window_fst of the
same O.Cfg(n1p, n2p, variant_type, fold, start, end), window by window: integers exact (chrom, begin, end,
snp_count -- variant_type matches only -- n2, n2_all, n1a, n1b), T values by golden_util.close where the
oracle has a value and None (sfs2d.post._v) exactly where it has None, Fst within 1e-12 + 1e-10 |x| (k_prep's
fixed point rounds each SNP's term by at most 2^-49 at these window sizes).

The genome's chromosomes hold LENGTHS SNPs, so the later ones start at offsets that are no multiple of 4,
and SFS2D_TILE = 4096 makes every tile edge a step edge (a step is 2,048 SNPs, 4 per lane).  Tiles start
at the multiple of 4 below the chromosome's first SNP: the filter edges are placed relative to that."""
import numpy as np
import pytest

import golden_util as gu
from oracle import sfs_oracle as O

pytestmark = pytest.mark.gpu

LENGTHS = [1, 7, 9, 2047, 2049, 4097, 3 * 4096 + 5]
TILE, STEP = 4096, 2048
WS = 20000
VT = "intron_variant"
MID_FIRST = 2 * STEP + 4 * 10 + 2      # third SNP of lane 10's four, in a tile's first step
MID_LAST = 3 * STEP + 4 * 37 + 1       # second SNP of lane 37's four, in a tile's second step
_DATA, _REF = {}, {}


@pytest.fixture(autouse=True)
def _small_tiles(monkeypatch):
    monkeypatch.setenv("SFS2D_TILE", str(TILE))
    for k in ("SFS2D_GW", "SFS2D_FUSED"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------- data sets

def _data(name):
    if name not in _DATA:
        # (fst_dense: the dense-window cases' oracle costs ~1 ms per window, so they leave out the middle
        # chromosomes -- the long one then starts at SNP 17, its tiles at 16)
        _DATA[name] = {"lengths": _lengths_genome, "fst": _fst_genome, "long_windows": _long_window_chrom,
                       "fst_dense": lambda: _fst_genome().subset_chroms([0, 1, 2, len(LENGTHS) - 1]),
                       "grid50": lambda: _large_grid_genome(50, 50), "grid100": lambda: _large_grid_genome(100, 75)}[name]()
    return _DATA[name]


def _lengths_genome():
    """Chromosomes of LENGTHS SNPs, three annotations, pop 25 / 25; the one-SNP chromosome's SNP is
    monomorphic (a window whose T2D is None in every case, the neutral filter included)."""
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_genome
    p = synth_genome(len(LENGTHS), LENGTHS, 25, 25, seed=5, n_ann=3)
    counts = p.counts.copy()
    counts[0] = int(pack_counts(np.array([50]), np.array([0]), np.array([50]), np.array([0]))[0])
    return PackedSNPs(counts, p.pos, p.chrom_off, list(p.chrom_names), p.ann_id, list(p.ann_names), p.pop1, p.pop2)


def _fst_genome():
    """The lengths genome with Fst's edge values written over every 37th SNP: a = 0, 1 and n in either
    population, and SNPs with fewer than 2 called alleles in a population (test_scan_variants'
    _fst_edge_chrom, low_nc)."""
    from sfs2d.pack import PackedSNPs, pack_counts
    p = _lengths_genome()
    edge = [(50, 0, 49, 1), (49, 1, 50, 0), (0, 50, 25, 25), (25, 25, 0, 50), (0, 50, 49, 1), (49, 1, 0, 50),
            (50, 0, 0, 50), (0, 50, 50, 0), (1, 1, 25, 25), (0, 2, 30, 20), (2, 0, 1, 1),
            (1, 0, 25, 25), (0, 1, 25, 25), (25, 25, 0, 1), (0, 0, 25, 25), (25, 25, 0, 0), (0, 1, 0, 1)]
    counts = p.counts.copy()
    at = np.arange(11, p.n, 37)
    e = np.array([edge[k % len(edge)] for k in range(len(at))])
    counts[at] = pack_counts(e[:, 0], e[:, 1], e[:, 2], e[:, 3])
    return PackedSNPs(counts, p.pos, p.chrom_off, list(p.chrom_names), p.ann_id, list(p.ann_names), p.pop1, p.pop2)


def _filters(p):
    """{name: (start, end)}: each bound is a SNP's own position (both compares are inclusive), the SNP
    counted from the long chromosome's first tile edge."""
    cb = int(p.chrom_off[-2])
    base = cb & ~3
    assert base + 2 * TILE + 1 < p.n
    at = lambda k: int(p.pos[base + k])
    short_last = max(int(p.pos[int(p.chrom_off[c + 1]) - 1]) for c in range(p.nchrom - 1))
    assert short_last + 1 < int(p.pos[-1]) and at(TILE) > 0
    return {"tile_first": (at(TILE), at(2 * TILE - 1)),          # a tile's first SNP .. a tile's last SNP
            "lane_second": (at(TILE + 1), at(2 * TILE)),         # the second of a lane's four .. a tile's first
            "mid_lane": (at(MID_FIRST), at(MID_LAST)),
            "start_only": (at(TILE + 1), None),
            "end_only": (None, at(2 * TILE - 1)),
            "short_empty": (short_last + 1, None),               # the short chromosomes' backgrounds are empty
            "nothing": (at(2 * TILE - 1), at(TILE)),             # end < start
            "neutral": (0, 2 ** 32 - 1)}                         # a bins plan in which everything passes


FILTERS = ["tile_first", "lane_second", "mid_lane", "start_only", "end_only", "short_empty", "nothing", "neutral"]


def _long_window_chrom():
    """test_scan_variants' _one_bin_chrom with a non-matching SNP (another in-grid bin) interleaved as every
    fifth: 20 kb windows of mixed SNPs | 511 | (empty slot) | 512 | 513 | monomorphic | 1025 matching SNPs in
    one bin (638 .. 1281 SNPs: streamed rows, ranks up to the D table's last entries) | mixed, then windows
    of 511, 512 and 513 SNPs in all (every fifth replaced: the first 8 rows' edge) and a mixed one."""
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(11))
    _, r1, a1, r2, a2 = synth_chrom(rng, 500, 25, 25)
    mixed = pack_counts(r1, a1, r2, a2)
    word = lambda x1, x2: int(pack_counts(np.array([50 - x1]), np.array([x1]), np.array([50 - x2]), np.array([x2]))[0])
    other = word(5, 5)

    def ins(c):   # a non-matching SNP after every four
        c = np.asarray(c, np.uint32)
        n = len(c) + len(c) // 4
        out, ann = np.full(n, other, np.uint32), np.zeros(n, np.uint16)
        keep = np.arange(n) % 5 != 4
        out[keep], ann[keep] = c, 1
        ann[~keep] = 2 * (np.arange((~keep).sum()) % 2)
        return out, ann

    def rep(c):   # every fifth SNP replaced by a non-matching one
        c = np.asarray(c, np.uint32).copy()
        ann = np.ones(len(c), np.uint16)
        c[4::5], ann[4::5] = other, 0
        return c, ann

    full = lambda n, w: np.full(n, w, np.uint32)
    layout = [(0, ins(mixed[:300])), (1, ins(full(511, word(3, 7)))), (3, ins(full(512, word(10, 2)))),
              (4, ins(full(513, word(1, 1)))), (5, ins(full(100, word(0, 0)))), (6, ins(full(1025, word(20, 24)))),
              (7, ins(mixed[300:])), (8, rep(full(511, word(2, 9)))), (9, rep(full(512, word(4, 4)))),
              (10, rep(full(513, word(6, 1)))), (11, rep(mixed[100:400]))]
    counts, ann, pos = [], [], []
    for w, (c, a) in layout:
        n = len(c)
        counts.append(c)
        ann.append(a)
        pos.append(w * WS + 1 + np.arange(n, dtype=np.int64) * (19000 // n))
    counts = np.concatenate(counts)
    return PackedSNPs(counts, np.concatenate(pos).astype(np.uint32), np.array([0, len(counts)], np.int64), ["chr0000"],
                      np.concatenate(ann), ["intergenic_region", VT, "missense_variant"], "p1", "p2")


GRID_WS = 30000


def _large_grid_genome(n1p, n2p):
    """About 4,000 SNPs in three chromosomes; the first 320 SNPs of one 30 kb window of >= 400 SNPs match the
    annotation and share one 2D bin (k_scan_gw's byte counters wrap: the exact path)."""
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_genome
    p = synth_genome(3, [2600, 1100, 300], n1p, n2p, seed=97 + n1p, n_ann=3)
    big = [w for w in O.bp_windows(p, GRID_WS) if w[0] == 0 and w[3] - w[2] >= 400 and w[2] >= 5 and w[2] + 320 <= 2000]
    b = big[0][2]   # (inside the position filter test_large_grids_filtered sets: SNPs 5 .. 2000)
    counts, ann = p.counts.copy(), p.ann_id.copy()
    counts[b:b + 320] = int(pack_counts(np.array([2 * n1p - 3]), np.array([3]), np.array([2 * n2p - 2]), np.array([2]))[0])
    ann[b:b + 320] = p.ann_names.index(VT)
    q = PackedSNPs(counts, p.pos, p.chrom_off, list(p.chrom_names), ann, list(p.ann_names), p.pop1, p.pop2)
    q.wrap_window = (b, b + 320)
    return q


# -------------------------------------------------------------------------------------------- oracle

def _props(wins, orec):
    """(some window's T2D is None, some window's is finite, some window's snp_count < its SNPs)."""
    return (any(o["T2D"] is None for o in orec),
            any(o["T2D"] is not None and np.isfinite(o["T2D"]) for o in orec),
            any(o["snp_count"] < w[-1] - w[-2] for w, o in zip(wins, orec)))


def _no_cancelled_t(values):
    """No oracle T in (0, 1e-2): a T is a sum of terms up to ~2e4 here, so any evaluation order, the oracle's
    included, carries an absolute rounding error of ~1e-12, which 1e-10 relative covers only from 1e-2 on
    (test_prep_step._cpu_check).  The seeds are fixed so that this holds."""
    for v in values:
        assert v is None or v == 0.0 or not np.isfinite(v) or abs(v) >= 1e-2, v


def _oracle(data, n1p, n2p, vt, fold, start, end, snps, w, finite_ok=True):
    """(windows, records, Fst, backgrounds) of every window, computed once per case and shared; the
    fixture's own properties are asserted here, on the CPU."""
    key = (data, n1p, n2p, vt, fold, start, end, snps, w)
    if key not in _REF:
        p = _data(data)
        ocfg = O.Cfg(n1p, n2p, vt, fold, start, end)
        bgs = O.chrom_backgrounds(p, ocfg)
        wins = O.snp_windows(p, w)[0] if snps else O.bp_windows(p, w)
        recs = O.window_records(p, wins, ocfg, lambda c: bgs[c])
        fst = [O.window_fst(p, np.arange(x[-2], x[-1]), ocfg) for x in wins]
        _no_cancelled_t(o[t] for o in recs for t in ("T2D", "T1D_p1", "T1D_p2"))
        has_none, has_finite, has_fewer = _props(wins, recs)
        # (what a case cannot hold: a finite T2D when nothing passes; snp_count < SNPs without variant_type,
        # which is all snp_count looks at)
        assert has_none and has_finite == finite_ok and has_fewer == (vt is not None), (key, has_none, has_finite, has_fewer)
        _REF[key] = (wins, recs, fst, bgs)
    return _REF[key]


# --------------------------------------------------------------------------------------------- checks

def _cfg(p, n1p, n2p, vt, fold, start, end, snps, w, **kw):
    from sfs2d import _lib as L
    from sfs2d.engine import ScanConfig
    return ScanConfig(n1p=n1p, n2p=n2p, fold=fold, window_mode=L.WINDOW_SNPS if snps else L.WINDOW_BP, window=w,
                      ann_want=-1 if vt is None else p.ann_names.index(vt), start_position=start, end_position=end, **kw)


def _run(p, cfg, runs=1, kernel=None):
    """`runs` runs of one plan: [(records, Fst or None), ...], exact-path windows counted so far."""
    from sfs2d.engine import Engine
    eng = Engine.get(0)
    dev = eng.upload(p)
    pl = eng.plan(dev, cfg)
    if kernel is not None:
        assert pl.scan_kernel() == kernel, pl.scan_kernel()
    out = []
    for _ in range(runs):
        pl.run()
        pl.check()
        out.append((pl.read(), pl.read_fst() if cfg.fst else None))
    exact = pl.stats()
    pl.close()
    dev.close()
    return out, exact


def _check(recs, fst, ref):
    from sfs2d import _lib as L
    from sfs2d import post
    wins, orec, ofst, _ = ref
    live = (recs["flags"] & L.W_EMPTY) == 0
    body = recs[live]
    assert len(body) == len(wins), (len(body), len(wins))
    if fst is not None:
        assert len(fst) == len(recs)
        assert np.all(np.isnan(fst[~live]))
        fl = fst[live]
    for i, (w, r, o) in enumerate(zip(wins, body, orec)):
        assert (int(r["chrom"]), int(r["begin"]), int(r["end"])) == (w[0], w[-2], w[-1]), (i, w)
        for a, b in (("snp_count", "snp_count"), ("n2", "N2"), ("n2_all", "N2_all"), ("n1a", "N1a"), ("n1b", "N1b")):
            assert int(r[a]) == o[b], (i, a, int(r[a]), o[b])
        for which, b in ((2, "T2D"), (1, "T1D_p1"), (0, "T1D_p2")):
            v = post._v(r, which)
            assert (v is None) == (o[b] is None), (i, b, v, o[b])
            assert gu.close(v, o[b]), (i, b, v, o[b])
        if fst is not None:
            g, f = float(fl[i]), ofst[i]
            assert (np.isnan(g) if f is None else abs(g - f) <= 1e-12 + 1e-10 * abs(f)), (i, "fst", g, f)


def _same_bytes(runs):
    for r, f in runs[1:]:
        assert r.tobytes() == runs[0][0].tobytes()
        assert f is None or f.tobytes() == runs[0][1].tobytes()


INTS = ("chrom", "wid", "begin", "end", "snp_count", "n2", "n2_all", "n1a", "n1b", "flags")


# ---------------------------------------------------------------------------------------------- tests

@pytest.mark.parametrize("name", FILTERS)
def test_filter_edges_on_kernel_edges(name):
    """(a) The first / last passing SNP on a tile's first SNP, the second of a lane's four, mid-lane, a
    tile's last SNP; one-sided filters; short chromosomes with an empty background; nothing passing; the
    neutral filter (a bins plan whose integers are the unfiltered plan's).  With and without variant_type,
    folded and not; a second run of the same plan byte-equal (bins buffer, replica parity, slot rewrite)."""
    p = _data("lengths")
    start, end = _filters(p)[name]
    for vt in ((None,) if name == "neutral" else (None, VT)):
        for fold in (True, False):
            ref = _oracle("lengths", 25, 25, vt, fold, start, end, False, WS, finite_ok=name != "nothing")
            if name == "short_empty":   # flags and None as the oracle's: every window of the short chromosomes
                assert all(o["T2D"] is None and o["T1D_p1"] is None for w, o in zip(ref[0], ref[1]) if w[0] < p.nchrom - 1)
            runs, _ = _run(p, _cfg(p, 25, 25, vt, fold, start, end, False, WS), runs=2, kernel="k_scan_w")
            _same_bytes(runs)
            _check(runs[0][0], None, ref)
            if name == "neutral":
                plain, _ = _run(p, _cfg(p, 25, 25, None, fold, None, None, False, WS))
                for k in INTS:
                    assert np.array_equal(runs[0][0][k], plain[0][0][k]), k


@pytest.mark.parametrize("name", FILTERS)
def test_bg_hist_filtered(name):
    """(b) Engine.bg_hist, the histogram-only pass k_prep<bg, no seg, lds, no bins, filter, no Fst>, with
    the same filters: every chromosome's histograms exactly O.chrom_backgrounds'."""
    import twoDSFS_class as T
    from sfs2d.engine import Engine
    p = _data("lengths")
    start, end = _filters(p)[name]
    eng = Engine.get(0)
    dev = eng.upload(p)
    for vt in ((None,) if name == "neutral" else (None, VT)):
        for fold in (True, False):
            bgs = _oracle("lengths", 25, 25, vt, fold, start, end, False, WS, finite_ok=name != "nothing")[3]
            cfg = _cfg(p, 25, 25, vt, fold, start, end, False, WS)
            for c in range(p.nchrom):
                h2, u1, u2 = eng.bg_hist(dev, cfg, c)
                assert np.array_equal(np.asarray(h2), np.asarray(bgs[c][0])), (vt, fold, c)
                assert np.array_equal(T._fold_counts(u1), np.asarray(bgs[c][1])), (vt, fold, c)
                assert np.array_equal(T._fold_counts(u2), np.asarray(bgs[c][2])), (vt, fold, c)
    dev.close()


@pytest.mark.parametrize("fused", ["0", "1"])
def test_long_windows_through_the_bins_rows(monkeypatch, fused):
    """(c) k_scan_w's non-CNT rows: windows past 512 SNPs (streamed rows: `lim` masking, plain loads) and of
    511 / 512 / 513 SNPs (the first 8 rows' edge), ranks reaching the D table's last entries, nvar < nsnp in
    every sized window, a monomorphic window and an empty slot; Fst from the bins words."""
    monkeypatch.setenv("SFS2D_FUSED", fused)
    p = _data("long_windows")
    ref = _oracle("long_windows", 25, 25, VT, True, None, None, False, WS)
    wins, orec = ref[0], ref[1]
    assert [w[3] - w[2] for w in wins] == [375, 638, 640, 641, 125, 1281, 250, 511, 512, 513, 300]
    assert [o["N2"] for o in orec[1:6]] == [511, 512, 513, 0, 1025]
    assert [o["N2"] for o in orec[7:10]] == [409, 410, 411]
    assert all(o["snp_count"] < w[3] - w[2] for w, o in zip(wins, orec))
    for cap in (0, 1):
        runs, _ = _run(p, _cfg(p, 25, 25, VT, True, None, None, False, WS, fst=True, scan_wgs_per_cu=cap), runs=2,
                       kernel="k_scan_w")
        _same_bytes(runs)
        assert len(runs[0][0]) == 12   # slot 2 is empty
        _check(runs[0][0], runs[0][1], ref)


@pytest.mark.parametrize("gw", ["1", "0"])
@pytest.mark.parametrize("data,n1p,n2p", [("grid50", 50, 50), ("grid100", 100, 75)])
def test_large_grids_filtered(monkeypatch, data, n1p, n2p, gw):
    """(d) k_scan_gw and k_scan_g without CNT: a position and variant_type filter on grids > 8192 bins, one
    window with 320 matching SNPs in one bin (k_scan_gw's u8 counters wrap: its exact path), with and
    without Fst."""
    monkeypatch.setenv("SFS2D_GW", gw)
    p = _data(data)
    b, e = p.wrap_window
    start, end = int(p.pos[5]), int(p.pos[2000])
    assert start <= int(p.pos[b]) and int(p.pos[e - 1]) <= end
    ref = _oracle(data, n1p, n2p, VT, True, start, end, False, GRID_WS)
    assert max(o["N2"] for o in ref[1]) >= 300
    for fst in (False, True):
        runs, exact = _run(p, _cfg(p, n1p, n2p, VT, True, start, end, False, GRID_WS, fst=fst), runs=2,
                           kernel="k_scan_gw" if gw == "1" else "k_scan_g")
        # (eval_exact sums a bin's term in whichever lane takes the bin, so a T's last bits may differ from run
        # to run: the second run's integers and Fst are the first's, and both runs are the oracle's)
        for k in INTS:
            assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
        for r, f in runs:
            _check(r, f, ref)
        if fst:
            assert runs[0][1].tobytes() == runs[1][1].tobytes()
        if gw == "1":
            assert exact > 0


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("snps,w", [(False, WS), (True, 7), (False, 335)])
def test_fst_on_filtered_plans(monkeypatch, snps, w, fused):
    """(e) Fst with a position filter and variant_type: k_prep's own fixed-point sums (SFS2D_FUSED=1, and
    SNP-count windows) and k_fst_win / k_bg_slice's Fst workgroups (SFS2D_FUSED=0, fixed-bp), which take
    membership from the bins words.  S = 7 (a lane's four SNPs straddle windows, the tail is dropped) and
    335 bp windows of ~6 SNPs put more than FST_LDS = 256 windows in a 4,096-SNP tile: the sums past them go
    to the global table.  SNPs with fewer than 2 called alleles in a population are sprinkled in; a SNP that
    fails a filter contributes nothing."""
    monkeypatch.setenv("SFS2D_FUSED", fused)
    data = "fst" if w == WS else "fst_dense"
    p = _data(data)
    start, end = _filters(p)["lane_second"]
    ref = _oracle(data, 25, 25, VT, True, start, end, snps, w)
    if w != WS:   # more windows in a tile than k_prep's LDS sums hold
        assert sum(1 for x in ref[0] if x[0] == p.nchrom - 1) > 3 * 256
    runs, _ = _run(p, _cfg(p, 25, 25, VT, True, start, end, snps, w, fst=True), runs=2, kernel="k_scan_w")
    _same_bytes(runs)
    _check(runs[0][0], runs[0][1], ref)


@pytest.mark.parametrize("S", [64, 500])
def test_filtered_snp_windows_through_the_class(S):
    """(f) scan_perChr_bySNPs of the drop-in class with variant_type and an end filter on a window's last
    SNP: the long chromosome's later windows hold no passing SNP (n2_all == 0) and are skipped by both
    sides; keys and values as O.scan_perChr_bySNPs."""
    import twoDSFS_class as T
    p = _data("lengths")
    cb = int(p.chrom_off[-2])
    end = int(p.pos[cb + S * (8000 // S) - 1])
    ocfg = O.Cfg(25, 25, VT, True, None, end)
    key = ("bysnps", S)
    if key not in _REF:
        _REF[key] = O.scan_perChr_bySNPs(p, S, ocfg)
    want = _REF[key]
    _no_cancelled_t(d[t] for d in want.values() for t in ("T2D", "T1D_pop1", "T1D_pop2"))
    nwin = len(O.snp_windows(p, S)[0])
    assert 0 < len(want) < nwin   # some windows kept, some skipped
    obj = T.LikelihoodInference_jointSFS(None, None, end_position=end, pop1=p.pop1, pop2=p.pop2, pop1_size=25,
                                         pop2_size=25, variant_type=VT)
    assert gu.compare_results(obj.scan_perChr_bySNPs(p, S), want) == []
