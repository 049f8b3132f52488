"""The fixtures of test_after_run_gpu.py (tests/after_util.py), on the oracle and the numpy twins alone: two data sets
with the same host-side facts that differ enough, window by window and background by background, for a post-scan
call that reads a stale buffer to give other bytes."""
import numpy as np
import pytest

import after_util as AU
import project_util as PU
from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import null as N


@pytest.mark.parametrize("which", ["small", "large"])
def test_pairs_share_every_host_side_fact(which):
    a, b = AU.pair(which)
    assert a.n == b.n == (14057 if which == "small" else 3306)
    assert np.array_equal(a.chrom_off, b.chrom_off) and a.chrom_names == b.chrom_names and a.ann_names == b.ann_names
    for c in range(a.nchrom):
        lo, hi = int(a.chrom_off[c]), int(a.chrom_off[c + 1])
        assert (a.pos[lo], a.pos[hi - 1]) == (b.pos[lo], b.pos[hi - 1])            # chrom_last_pos unchanged
        assert (np.diff(b.pos[lo:hi].astype(np.int64)) > 0).all()                  # strictly increasing
    # the same multiset of (counts, annotation) pairs; the largest called counts with it
    key = lambda p: np.sort(p.counts.astype(np.uint64) << np.uint64(16) | p.ann_id.astype(np.uint64))
    assert np.array_equal(key(a), key(b))
    assert not np.array_equal(a.counts, b.counts) and not np.array_equal(a.pos, b.pos)


@pytest.mark.parametrize("kind", list(AU.KINDS))
def test_records_differ_between_a_and_b(kind):
    a, b = AU.pair(AU.which_of(kind))
    (sa, ra), (sb, rb) = AU.slot_records(kind, a), AU.slot_records(kind, b)
    assert len(sa) == len(sb) > 5                                                  # slot i of A is slot i of B
    assert [s[:2] for s in sa] == [s[:2] for s in sb]
    live = [i for i in range(len(sa)) if ra[i] is not None or rb[i] is not None]
    assert len(live) >= 10
    cfg = AU.record_config(kind)
    if cfg.window_mode == L.WINDOW_BP:
        moved = sum(sa[i][2:] != sb[i][2:] for i in live)
        assert 2 * moved > len(live), (moved, len(live))
    # (a window that the position filter leaves without a member has n2 = 0 and no T in either data set: the records
    # compared are the ones with a member of the SFS in A or in B)
    live = [i for i in live if any(r[i] is not None and r[i]["N2_all"] > 0 for r in (ra, rb))]
    assert len(live) >= 10
    other = sum(ra[i] is None or rb[i] is None or ra[i]["N2"] != rb[i]["N2"] or ra[i]["T2D"] != rb[i]["T2D"] for i in live)
    assert 10 * other > 9 * len(live), (other, len(live))


@pytest.mark.parametrize("kind", ["fused", "gw", "filtered"])
def test_backgrounds_differ_between_a_and_b(kind):
    a, b = AU.pair(AU.which_of(kind))
    cfg = AU.scan_config(kind)
    ba, bb = O.chrom_backgrounds(a, AU.oracle_cfg(cfg, a)), O.chrom_backgrounds(b, AU.oracle_cfg(cfg, b))
    seen = 0
    for c in range(a.nchrom):
        if int(a.chrom_off[c + 1] - a.chrom_off[c]) >= 255:
            assert not np.array_equal(ba[c][0], bb[c][0]), c
            seen += 1
    assert seen >= 3


@pytest.mark.parametrize("block", [1, AU.NULL_BLOCK])
def test_null_draws_reach_the_last_inner_bin_in_b(block):
    """Without a drawn SNP in the last inner 2D bin a background table without its tail gives the same T."""
    b = AU.pair("small")[1]
    n1p, n2p = AU.N_SMALL
    cfg = O.Cfg(n1p, n2p)
    tasks = AU.tasks("small")
    q, wins = N.resample(b, tasks, AU.NULL_REPS, AU.NULL_SEED, block=block)
    assert len(wins) == len(tasks) * AU.NULL_REPS
    hit = [w for w in wins if O.sfs2d(q, np.arange(w[-2], w[-1]), cfg)[2 * n1p, 2 * n2p - 1] > 0]
    assert hit
    bgs = O.chrom_backgrounds(b, cfg)
    assert all(bgs[w[0]][0][2 * n1p, 2 * n2p - 1] > 0 for w in hit)                # (a bin of the pool's own background)


def test_planted_kinds_survive():
    n1p, n2p = AU.N_SMALL
    for p in AU.pair("small"):
        PU.assert_kinds(p, n1p, n2p, *AU.M_SMALL)
        PU.assert_dropped_share(p, PU.Cfg(n1p, n2p), *AU.M_SMALL)
