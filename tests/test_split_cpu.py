"""The in-process split driver (tests/split_util.py) and the fixtures of test_split_gpu.py, on the oracle alone (no
GPU): the driver with dist_worker.FakeSplitJob parts gives the table the oracle gives for the whole data set, for
every (data set, config, cut list) the GPU tests split, and the fixtures hold what those tests say they hold."""
import numpy as np
import pytest

import dist_worker as DW
import split_util as SU
from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import dist as D

CASES = SU.all_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_driver_equals_whole_oracle_scan(name):
    """Byte-equal to dist_worker.fake_scan of the whole data set (empty slots dropped, the helper's wid zeroed);
    the summed rows are the whole data set's rows; every cut is a window start of the config."""
    p, cfg = CASES[name]
    whole = SU.strip(DW.fake_scan(p, cfg, None))
    want_rows = DW.FakeSplitJob(p, cfg, None).partial()
    starts = set(D.window_starts(p, cfg).tolist()) | {0, p.n}
    for cname, cuts in SU.cut_lists(p, cfg).items():
        assert all(c in starts for c in cuts), (cname, cuts)
        res = SU.fake_split((name, cname), p, cfg, cuts)
        assert SU.strip(res.table).tobytes() == whole.tobytes(), cname
        assert np.array_equal(res.total, want_rows)
        assert [r is None for r in res.rows] == [cuts[i + 1] == cuts[i] for i in range(len(cuts) - 1)]
    assert len(whole) >= 6 and (whole["flags"] & L.W_EXTRA != 0).sum() == int(bool(cfg.prev_extra))


def test_driver_stride_padding():
    """A stride above the row width: the padding words stay -1 in every part's rows and sum to -K."""
    p, cfg = CASES["rows-10x30-fold"]
    W = D.hist_width(cfg)
    cuts = SU.four_cuts(p, cfg)
    res = SU.split_in_process(p, cfg, cuts, DW.FakeSplitJob, stride=W + 5)
    assert res.buffer.shape == (4, 3, W + 5) and np.all(res.buffer[:, :, W:] == -1) and np.all(res.total[:, W:] == -4)
    assert res.table.tobytes() == SU.fake_split(("rows-10x30-fold", "four"), p, cfg, cuts).table.tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cut_lists(name):
    """Four parts: chromosome 0 in parts 0-1, chromosome 1 in parts 1-2, chromosome 2 alone in part 3; the other
    list repeats the middle cut (an empty part 2); with the Q9 helper the last part keeps >= 2 windows."""
    p, cfg = CASES[name]
    lists = SU.cut_lists(p, cfg)
    c = lists["four"]
    off = [int(x) for x in p.chrom_off]
    assert len(c) == 5 and c[0] == 0 and off[0] < c[1] < off[1] < c[2] < off[2] == c[3] < off[3] == c[4]
    assert [p.slice_snps(c[r], c[r + 1])[1] for r in range(4)] == [0, 0, 1, 2]
    assert [p.slice_snps(c[r], c[r + 1])[0].nchrom for r in range(4)] == [1, 2, 1, 1]
    e = lists["empty"]
    assert e == c[:3] + c[2:] and len(e) == 6 and e[2] == e[3]
    assert abs(c[1] - off[1] / 3) < 600 and abs(c[2] - (off[1] + off[2]) / 2) < 700   # near the rule's targets
    if cfg.prev_extra:
        assert len(SU.windows(p.slice_snps(c[3], c[4])[0], cfg)) >= 2


def test_grids_take_the_paths_claimed():
    """The large grids are above k_scan_w's 8,192 2D bins and the small ones below; the row grids are asymmetric
    (a transposed or mis-offset row cannot pass) and their three row segments have three different lengths."""
    for n1p, n2p in SU.GRIDS_LARGE:
        assert (2 * n1p + 1) * (2 * n2p + 1) > 8192
    for n1p, n2p in ((25, 25), (10, 30)):
        assert (2 * n1p + 1) * (2 * n2p + 1) <= 8192
    assert sum(a != b for a, b in SU.GRIDS_ROWS) == 2
    for n1p, n2p in SU.GRIDS_ROWS:
        rows = DW.FakeSplitJob(SU.genome(n1p, n2p), SU.bp_cfg(n1p, n2p), None).partial()
        assert rows.shape == (3, L.bg_row_words(n1p, n2p))
        nb = (2 * n1p + 1) * (2 * n2p + 1)
        h2 = rows[0, :nb].reshape(2 * n1p + 1, 2 * n2p + 1)
        if n1p != n2p:   # a transposed 2D block differs
            assert not np.array_equal(h2.T.ravel(), rows[0, :nb])
        assert rows[0, nb:nb + 2 * n1p + 1].sum() > 0 and rows[0, nb + 2 * n1p + 1:-1].sum() > 0
        assert rows[0, -1] == rows[0, 1:nb - 1].sum() > 0


def test_row_variants_differ():
    """Fold, variant_type and the position filter each change the rows; the position filter cuts chromosomes 0
    and 1 on both sides and empties chromosome 2 (its total inner sum is 0: BG2_ZERO windows)."""
    for n1p, n2p in SU.GRIDS_ROWS:
        p = SU.genome(n1p, n2p)
        rows = {v: DW.FakeSplitJob(p, cfg, None).partial() for v, cfg in SU.row_variants(n1p, n2p).items()}
        assert len({r.tobytes() for r in rows.values()}) == 4
        s, e = SU.filter_positions(p)
        for c in (0, 1):
            pos = p.pos[p.chrom_off[c]:p.chrom_off[c + 1]].astype(np.int64)
            assert (pos < s).sum() > 100 and (pos > e).sum() > 100 and ((pos >= s) & (pos <= e)).sum() > 100
        assert rows["pos"][2].sum() == 0 and rows["pos"][0, -1] > 0 and rows["pos"][1, -1] > 0
        assert 0 < rows["ann"][0, -1] < rows["fold"][0, -1]


def test_wide_case_has_a_cut_inside_chromosome_1():
    p, cfg = CASES["wide-70k"]
    c = SU.four_cuts(p, cfg)
    assert int(p.pos[c[2]]) > 70000 >= int(p.pos[c[2] - 1])
    p, cfg = CASES["attach-100k"]
    c = SU.four_cuts(p, cfg)
    assert int(p.pos[c[1]]) > 100000 >= int(p.pos[c[1] - 1]) and int(p.pos[c[2]]) > 100000 >= int(p.pos[c[2] - 1])
    base = set(D.window_starts(p, SU.bp_cfg(25, 25)).tolist())   # the attached plan's cuts are the base's too
    assert all(x in base or x == p.n for x in c)


def _part_inner(res, r):
    return res.rows[r][:, -1]


def test_corner_part_fixture():
    """Part 2 (the second half of chromosome 1): every SNP in (0, 0) or (n1, n2) of the unfolded grid, so its own
    inner 2D sum and inner folded 1D sums are 0 although it holds SNPs in the last bin; the chromosome's totals
    are not 0, and the oracle's table has no BG*_ZERO flag on chromosome 1."""
    p, cfg = CASES["corner_part"]
    cuts = SU.four_cuts(p, cfg)
    assert cuts == SU.four_cuts(SU.genome(25, 25), cfg)
    res = SU.fake_split(("corner_part", "four"), p, cfg, cuts)
    row = res.rows[2][0]
    nb = 51 * 51
    assert row[-1] == 0 and row[nb - 1] == (cuts[3] - cuts[2]) // 2 > 100 and row[:nb - 1].sum() == 0
    assert row[nb + 50] == row[nb - 1] and row[nb:nb + 50].sum() == 0           # pop 1: all at alt = n1
    assert row[nb + 51 + 50] == row[nb - 1] and row[nb + 51:nb + 51 + 50].sum() == 0
    assert res.total[1, -1] > 0 and _part_inner(res, 1)[1] > 0
    t = res.table[res.table["chrom"] == 1]
    assert len(t) >= 4 and np.all(t["flags"] & 7 == 0)
    mine = t[t["begin"] >= cuts[2]]
    assert len(mine) >= 2 and np.all(mine["n2"] == 0) and np.all(mine["n2_all"] > 0) and np.all(mine["n1a"] == 0)


def test_zero_chrom_fixture():
    """Chromosome 1's total inner 2D sum is 0 over parts 1 and 2 (both hold SNPs of it); every window of it carries
    BG2_ZERO (and both 1D flags) in the oracle's table, no window of chromosomes 0 and 2 does."""
    p, cfg = CASES["zero_chrom"]
    cuts = SU.four_cuts(p, cfg)
    res = SU.fake_split(("zero_chrom", "four"), p, cfg, cuts)
    assert res.total[1, -1] == 0 and res.total[1, 51 * 51 - 1] > 1000
    assert _part_inner(res, 1)[0] > 0 and _part_inner(res, 1)[1] == 0 and _part_inner(res, 2)[0] == 0
    body = res.table[(res.table["flags"] & L.W_EXTRA) == 0]
    on1 = body["chrom"] == 1
    assert on1.sum() >= 4 and (body["begin"][on1] < cuts[2]).any() and (body["begin"][on1] >= cuts[2]).any()
    assert np.all(body["flags"][on1] & 7 == 7) and np.all(body["flags"][~on1] & 7 == 0)


def test_end_filter_fixture():
    """end_position at the last SNP before the middle cut: part 2's rows are all 0, chromosome 1's total is not;
    its windows count their SNPs (snp_count) but hold none in the SFS, and carry no BG*_ZERO flag."""
    p, cfg = CASES["end_filter"]
    cuts = SU.four_cuts(p, cfg)
    res = SU.fake_split(("end_filter", "four"), p, cfg, cuts)
    assert not res.rows[2].any() and res.total[1, -1] > 0 and res.rows[1][1, -1] == res.total[1, -1]
    t = res.table[(res.table["chrom"] == 1) & (res.table["begin"] >= cuts[2]) & ((res.table["flags"] & L.W_EXTRA) == 0)]
    assert len(t) >= 2 and np.all(t["snp_count"] > 0) and np.all(t["n2_all"] == 0) and np.all(t["flags"] & 7 == 0)


def test_matrix_windows_have_values():
    """Every matrix config has windows with all three statistics in every part, and no oracle T in (0, 1e-2)
    (wide_util.no_cancelled_t: golden_util.close is relative)."""
    import wide_util as U
    for name in ("w-bp20k-fst1", "w-snp500-fst1", "large-50x50", "large-60x35", "wide-70k", "attach-100k"):
        p, cfg = CASES[name]
        ocfg = SU.ocfg_of(p, cfg)
        bgs = O.chrom_backgrounds(p, ocfg)
        wins = SU.windows(p, cfg)
        ref = U.oracle_ref(p, wins, ocfg, lambda c: bgs[c], key=("split", name))
        U.no_cancelled_t(ref[1])
        cuts = SU.four_cuts(p, cfg)
        for r in range(4):
            mine = [o for w, o in zip(wins, ref[1]) if cuts[r] <= w[-2] < cuts[r + 1]]
            assert sum(1 for o in mine if None not in (o["T2D"], o["T1D_p1"], o["T1D_p2"])) >= 1, (name, r)
        assert sum(f is not None for f in ref[2]) >= len(wins) - 1


def test_parts_alone_have_values():
    """(c) runs each part's plan on its own after a split: against its own backgrounds every part keeps windows
    with all three statistics and no oracle T in (0, 1e-2)."""
    import wide_util as U
    for name in ("w-bp20k-fst1", "large-60x35"):
        p, cfg = CASES[name]
        res = SU.fake_split((name, "four"), p, cfg, SU.four_cuts(p, cfg))
        for r, sub in enumerate(res.subs):
            ocfg = SU.ocfg_of(sub, cfg)
            bgs = O.chrom_backgrounds(sub, ocfg)
            ref = U.oracle_ref(sub, SU.windows(sub, cfg), ocfg, lambda c: bgs[c], key=("split-part", name, r))
            U.no_cancelled_t(ref[1])
            assert U.full_windows(ref[1]) >= 2, (name, r)
