"""The fixtures of test_wide_bins.py and test_position_edges.py hold what those tests say they hold: asserted on
the oracle alone, so that a fixture cannot go quietly vacuous (no GPU)."""
import numpy as np

import test_position_edges as PE
import test_wide_bins as WB
import wide_util as U
from oracle import sfs_oracle as O


def _ordinary(ref, at_least=3):
    """>= 3 windows with all three statistics, and no oracle T in (0, 1e-2)."""
    assert U.full_windows(ref[1]) >= at_least, U.full_windows(ref[1])
    U.no_cancelled_t(ref[1])


def test_wide_bins_cases():
    """Every k_scan_w case: ~1,170-SNP windows far below 65,536 (only the missing host positions make them wide),
    windows with values, Fst values where the case asks for Fst; the over-called and low-called-count fixtures
    hold such SNPs."""
    for n1p, n2p, window, _, case in WB.W_PARAMS:
        p, cfg, ocfg, bg, wins, key, bg_of = WB.w_case(n1p, n2p, window, case)
        ref = U.oracle_ref(p, wins, ocfg, bg_of, key)
        _ordinary(ref, 6)
        assert len(wins) == (10 if window == WB.W1 else 6) and len([w for w in wins if w[0] == 0]) == (6 if window == WB.W1 else 3)
        assert 1000 < max(w[3] - w[2] for w in wins) < 3000
        if cfg.fst:
            assert sum(f is not None for f in ref[2]) >= 6
    p = WB.genome("over")
    assert max((p.ref1 + p.alt1).max(), (p.ref2 + p.alt2).max()) > 50
    q = WB.genome("lownc")
    assert np.minimum(q.ref1 + q.alt1, q.ref2 + q.alt2).min() < 2
    r = WB.genome("plain")
    assert (r.ref1 + r.alt1).max() <= 50 and np.minimum(r.ref1 + r.alt1, r.ref2 + r.alt2).min() >= 2
    for g in (p, q, r):   # wrapped data must keep the contract: strictly increasing positions
        for c in range(g.nchrom):
            assert np.all(np.diff(g.pos[g.chrom_off[c]:g.chrom_off[c + 1]].astype(np.int64)) > 0)


def test_wide_bins_large_grid_sliding_attached():
    for n1p, n2p in ((50, 50), (100, 75)):
        p = WB.genome("plain", n1p, n2p)
        ocfg = O.Cfg(n1p, n2p)
        bgs = O.chrom_backgrounds(p, ocfg)
        _ordinary(U.oracle_ref(p, O.bp_windows(p, WB.W1), ocfg, lambda c: bgs[c],
                               key=("w", "plain", n1p, n2p, WB.W1, None, True, None, None)), 6)
    p = WB.genome("plain")
    ocfg = O.Cfg(25, 25)
    bgs = O.chrom_backgrounds(p, ocfg)
    slots = U.sliding_slots(p, WB.W1, WB.W1 // 4)
    wins = [s for s in slots if s[2] < s[3]]
    assert len(wins) > 20
    _ordinary(U.oracle_ref(p, wins, ocfg, lambda c: bgs[c], key=("slide", WB.W1)), 20)
    _ordinary(U.oracle_ref(p, O.snp_windows(p, 300)[0], ocfg, lambda c: bgs[c], key=("snp", 300)), 20)
    _ordinary(U.oracle_ref(p, O.bp_windows(p, 16384), ocfg, lambda c: bgs[c],
                           key=("w", "plain", 25, 25, 16384, None, True, None, None)), 20)


def test_big_bin_fixture():
    """The first 40,000-bp window holds 300 + 66,000 + k SNPs and one 2D bin of >= 66,000; as SNP-count windows of
    70,000 the chromosome is one window with that bin; the big window's T2D is not in (-1e-2, 1e-2)."""
    p, ocfg, wins, ref = WB.big_bin_ref(False)
    n0 = wins[0][3] - wins[0][2]
    assert wins[0][0] == 0 and WB.BIG + 300 < n0 < WB.BIG + 400
    assert all(w[3] - w[2] < 1000 for w in wins[1:]) and len(wins) >= 6
    g = O.sfs2d(p, np.arange(wins[0][2], wins[0][3]), ocfg)
    assert g.max() >= WB.BIG >= 65536 and g[3, 20] == g.max()
    assert abs(ref[1][0]["T2D"]) >= 1e-2
    _ordinary(ref)
    rl, _ = PE.run_lengths(p.pos[: p.chrom_off[1]])
    assert rl.max() == 4 and (rl == 4).sum() == WB.BIG // 4
    p, ocfg, wins, ref = WB.big_bin_ref(True)
    assert [(w[0], w[4] - w[3]) for w in wins] == [(0, WB.BIG_SNPS)]
    assert O.sfs2d(p, np.arange(wins[0][3], wins[0][4]), ocfg).max() >= WB.BIG
    assert abs(ref[1][0]["T2D"]) >= 1e-2 and U.full_windows(ref[1]) == 1


def test_duplicate_fixture():
    """Runs of 2 to 40 and one of 5,000; runs straddle multiples of 4 and of 64 and the k_prep tile edge at SNP
    2,048 (SFS2D_TILE = 2048); every plan geometry has windows with values; window = 7 stays under 65,536 slots
    and most of its windows hold one position's run."""
    p = PE.dup_genome()
    assert p.n == 9300 and list(p.chrom_off) == [0, 2600, 9000, 9300]
    rl, first = PE.run_lengths(p.pos)   # (no position is shared across a chromosome edge)
    assert sorted(set(rl))[0] == 1 and rl.max() == 5000 and sorted(set(rl))[-2] <= 40
    assert (rl > 1).sum() > 100 and (rl == 2).any() and ((rl >= 30) & (rl <= 40)).any()
    inside = lambda m: ((first < m) & (first + rl > m))   # a run holds SNPs on both sides of index m
    assert sum(inside(m).any() for m in range(4, p.n, 4)) > 100
    assert sum(inside(m).any() for m in range(64, p.n, 64)) > 20
    k = int(np.flatnonzero(inside(PE.DUP_TILE))[0])
    assert first[k] < PE.DUP_TILE < first[k] + rl[k] - 1 and rl[k] >= 3
    big = int(np.argmax(rl))
    assert 2600 < first[big] and first[big] + 5000 < 9000
    for c in range(p.nchrom):
        assert np.all(np.diff(p.pos[p.chrom_off[c]:p.chrom_off[c + 1]].astype(np.int64)) >= 0)
    for args in ((25, 25, PE.DUP_WS), (25, 25, PE.DUP_WS, PE.VT), (25, 25, PE.DUP_WS, None, PE.DUP_WS // 4),
                 (25, 25, 5 * PE.DUP_WS), (50, 50, PE.DUP_WS)):
        _ordinary(PE.dup_ref(*args)[3])
    assert max(w[3] - w[2] for w in PE.dup_ref(25, 25, PE.DUP_WS)[3][0]) > 5000
    p, ocfg, bgs, ref = PE.dup_ref(25, 25, 7)
    _ordinary(ref)
    one = sum(1 for w in ref[0] if p.pos[w[2]] == p.pos[w[3] - 1])
    assert one > 0.9 * len(ref[0]) and sum(1 for w in ref[0] if w[3] - w[2] > 1 and p.pos[w[2]] == p.pos[w[3] - 1]) > 100
    assert sum((int(p.pos[p.chrom_off[c + 1] - 1]) - 1) // 7 + 1 for c in range(3)) < 65536


def test_edge_fixture():
    """Positions 0, 0, 1 .. 4294967290, 4294967295, 4294967295; SNPs on both sides of the window edges named;
    65,536 slots at most on the chromosome; most slots empty; every window size has windows."""
    p = PE.edge_genome()
    pos = p.pos[:2000].astype(np.int64)
    assert list(pos[:3]) == [0, 0, 1] and list(pos[-3:]) == [4294967290, 4294967295, 4294967295]
    assert np.all(np.diff(pos) >= 0) and len(np.unique(pos)) == 1998
    for ws in PE.EDGE_WS:
        wid = np.where(pos > 0, (np.maximum(pos, 1) - 1) // ws, 0)
        nslots = int(wid[-1]) + 1
        assert nslots <= 65536 and (ws != 65536 or nslots == 65536)
        p_, ocfg, bgs, ref = PE.edge_ref(ws)
        assert len([w for w in ref[0] if w[0] == 0]) == len(np.unique(wid))
        assert nslots <= 4 or len(np.unique(wid)) < nslots // 10   # most of the axis is empty slots
        if nslots > 1:   # a window edge with SNPs at both the last position of a window and the first of the next
            edges = [(j + 1) * ws for j in range(min(nslots - 1, 3))]
            assert any(m in pos and m + 1 in pos for m in edges), ws
    assert sum(U.full_windows(PE.edge_ref(ws)[3][1]) for ws in PE.EDGE_WS) >= 3
    for ws in PE.EDGE_WS[:3]:
        _ordinary(PE.edge_ref(ws)[3])
    for S in (63, 64, 65, 2000):
        _ordinary(PE.edge_ref(S, snps=True)[3], 1)
    ref = PE.edge_ref(2 ** 31, step=2 ** 29)[3]
    _ordinary(ref)
    assert len(ref[0]) == 9


def test_million_fixture():
    """One window of 2^20 + 100 + k SNPs between two ordinary ones: its N, a bin of it, the chromosome's B and a
    background bin are all >= 2^20 (LNX_N); its T2D is not in (-1e-2, 1e-2); Fst's fixed point is 2^40 there and
    the bound on the big window's error is below the 1e-10 |x| every Fst gets."""
    for n1p, n2p in ((25, 25), (50, 50)):
        p, ocfg, bgs, ref = PE.million_ref(n1p, n2p)
        sizes = [(w[0], w[3] - w[2]) for w in ref[0]]
        assert [c for c, _ in sizes] == [0, 0, 0, 1]
        assert sizes[0][1] == 3000 and PE.MILLION < sizes[1][1] < PE.MILLION + 400 and sizes[2][1] > 2000
        o = ref[1][1]
        assert min(o["N2"], o["N1a"], o["N1b"]) >= 2 ** 20
        g = O.sfs2d(p, np.arange(ref[0][1][2], ref[0][1][3]), ocfg)
        assert g.max() >= PE.MILLION and bgs[0][0].max() >= PE.MILLION
        assert min(bgs[0][0].ravel()[1:-1].sum(), bgs[0][1][1:-1].sum(), bgs[0][2][1:-1].sum()) >= 2 ** 20
        assert abs(o["T2D"]) >= 1e-2
        assert U.full_windows(ref[1]) >= 3
        U.no_cancelled_t(ref[1])
        e, bound = PE.fst_fixed_point_bound(p, ref[0], ocfg)
        assert e == 40
        assert bound[1] < 1e-10 * abs(ref[2][1])   # (the big window)


def test_windows_of_fixed_alt_snps_only():
    """The one- and two-SNP windows and the 7-bp windows hold windows whose SNPs are all fixed for the alternative
    allele in both populations, at a called count n with n * (1 / n) != 1 in fp64: no SNP qualifies for Fst (None)
    although the 1D spectra hold SNPs -- the windows on which floating-point Fst sums left ~1e-16 instead of 0."""
    cases = [PE.edge_ref(1, snps=True), PE.edge_ref(2, snps=True), PE.dup_ref(25, 25, 7)]
    for p, ocfg, bgs, ref in cases:
        hit = 0
        for w, o, f in zip(*ref):
            idx = np.arange(w[-2], w[-1])
            if f is None and o["N1a"] > 0 and np.all(p.ref1[idx] + p.ref2[idx] == 0):
                n = np.concatenate([p.alt1[idx], p.alt2[idx]]).astype(np.float64)
                hit += bool(np.any(n * (1.0 / n) != 1.0))
        assert hit >= 1
