"""Block bootstrap null, host side (sfs2d.null, ``block``; DESIGN.md section 14, "blocks"): the host twin of
k_null_blk's draws -- runs of consecutive SNPs of a circular pool -- and the calibration that says why the
feature exists, with the oracle standing in for the device (no GPU).

Calibration data: the 20,000 i.i.d. SNPs of test_null_cpu's calibration, made linked by repeating SNPs in
runs of geometric length (mean 5): 400 windows of 50 SNPs, R = 999, null seed 0, sizes="exact".  The
single-SNP null (block 1) has no linkage, a window of ~10 distinct SNPs is over-dispersed against it and
almost every p_T2D is small; blocks as long as the window are a random placement of the window on the
chromosome, and p_T2D is uniform: Kolmogorov-Smirnov distance to U(0, 1) below 1.95 / sqrt(400) = 0.0975, the
0.1 % critical value."""
import math

import numpy as np
import pytest

import null_util as U
from oracle import sfs_oracle as O
from sfs2d import null as N
from sfs2d.pack import PackedSNPs
from sfs2d.synth import _philox, synth_genome


def _single_snp_draws(seed, pool_id, lo, n, m, replicates):
    """The single-SNP draws written out from their definition (what draw_indices was before it had blocks)."""
    j = np.arange(m, dtype=np.uint64)[None, :]
    r = np.arange(replicates, dtype=np.uint64)[:, None]
    q = np.broadcast_to(j >> np.uint64(1), (replicates, m))
    rr = np.broadcast_to(r, (replicates, m))
    c0, c1, c2, c3 = _philox(q, rr, np.uint64(m), np.uint64((pool_id + 1) & 0xFFFFFFFF), seed & 0xFFFFFFFF, seed >> 32)
    x = np.where((j & np.uint64(1)) == 0, c0 | (c1 << np.uint64(32)), c2 | (c3 << np.uint64(32)))
    return np.array([[lo + ((int(v) * n) >> 64) for v in row] for row in x], np.int64)


# ----------------------------------------------------------------------------- draws

@pytest.mark.parametrize("args", [(3, 1, 1000, 77, 129, 11), (5, -1, 0, 4205, 64, 3), (11 + (1 << 32), 0, 7, 1, 9, 2),
                                  (9, -1, 0, (1 << 32) - 1, 65, 2)])
def test_block_one_is_the_single_snp_null(args):
    a = N.draw_indices(*args)
    b = N.draw_indices(*args, block=1)
    assert a.dtype == b.dtype == np.int64 and a.tobytes() == b.tobytes()
    assert a.tobytes() == _single_snp_draws(*args).tobytes()


def test_block_one_resample_is_unchanged():
    p = synth_genome(3, [300, 5, 120], 3, 2, seed=1)
    tasks = [(0, 7), (2, 64), (1, 8)]
    q0, w0 = N.resample(p, tasks, 6, seed=11)
    q1, w1 = N.resample(p, tasks, 6, seed=11, block=1)
    assert w0 == w1
    for f in ("counts", "pos", "chrom_off", "ann_id"):
        assert getattr(q0, f).tobytes() == getattr(q1, f).tobytes(), f
    for t, (pool, m) in enumerate(tasks):
        lo, n = N.pool_range(p, pool)
        d = _single_snp_draws(11, pool, lo, n, m, 6)
        b, e = w0[t * 6][2], w0[t * 6 + 5][3]
        assert np.array_equal(q0.counts[b:e], p.counts[d.reshape(-1)])
    # and with blocks: each window is the drawn runs, every SNP with its own position and annotation
    q4, w4 = N.resample(p, tasks, 6, seed=11, block=4)
    assert w4 == w0
    d = N.draw_indices(11, 2, *N.pool_range(p, 2), 64, 6, block=4)
    b, e = w4[6][2], w4[11][3]
    assert np.array_equal(q4.counts[b:e], p.counts[d.reshape(-1)]) and np.array_equal(q4.pos[b:e], p.pos[d.reshape(-1)])
    assert np.array_equal(q4.ann_id[b:e], p.ann_id[d.reshape(-1)])


def test_pinned_block_vectors():
    assert N.draw_indices(5, 2, 3005, 1200, 10, 2, block=4).tolist() == [
        [3344, 3345, 3346, 3347, 3751, 3752, 3753, 3754, 3384, 3385],
        [3478, 3479, 3480, 3481, 3525, 3526, 3527, 3528, 3953, 3954]]
    # block starts 4 and 1 in a pool of 5: k reaches past n, the pool is circular, the last block is cut at m
    assert N.draw_indices(5, 1, 3000, 5, 9, 2, block=7)[0].tolist() == [3004, 3000, 3001, 3002, 3003, 3004, 3000, 3001, 3002]


def test_block_draws_depend_on_seed_pool_m_block_replicate_alone():
    lo, n, m = 3005, 1200, 129
    a = N.draw_indices(5, 2, lo, n, m, 6, block=7)
    assert a.shape == (6, m)
    assert np.array_equal(a[:2], N.draw_indices(5, 2, lo, n, m, 2, block=7))       # fewer replicates: the same first ones
    # b is not in the counter: block i of any block length starts where single-SNP draw i lies
    one = N.draw_indices(5, 2, lo, n, m, 6)
    for b in (2, 7, 64, 65):
        d = N.draw_indices(5, 2, lo, n, m, 6, block=b)
        nblk = -(-m // b)
        assert np.array_equal(d[:, ::b], one[:, :nblk]), b
        k = np.arange(m) % b
        assert np.array_equal(d, lo + (one[:, np.arange(m) // b] - lo + k) % n), b
    # any b >= m is one contiguous run from the same start
    run = N.draw_indices(5, 2, lo, n, m, 6, block=m)
    assert np.array_equal(run, lo + (one[:, :1] - lo + np.arange(m)) % n)
    for b in (m + 1, 700, (1 << 32) - 1):
        assert np.array_equal(N.draw_indices(5, 2, lo, n, m, 6, block=b), run)
    assert not np.array_equal(a, N.draw_indices(6, 2, lo, n, m, 6, block=7))
    assert not np.array_equal(a, N.draw_indices(5, 1, lo, n, m, 6, block=7))
    assert not np.array_equal(a[:, :128], N.draw_indices(5, 2, lo, n, 128, 6, block=7))


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("b", [7, 700])
def test_block_draws_stay_in_the_pool(n, b):
    for m in (1, 9, 700, 701):
        d = N.draw_indices(3, 1, 3000, n, m, 4, block=b)
        assert d.shape == (4, m) and d.min() >= 3000 and d.max() < 3000 + n
        assert np.all((d[:, 1:] - d[:, :-1])[:, (np.arange(1, m) % b) != 0] % n == 1 % n)   # inside a block: the next SNP
        if n == 5 and m >= 9:
            assert len(np.unique(d)) == 5


def test_argument_errors():
    for bad in (0, -1, 1 << 32):
        with pytest.raises(ValueError, match="block"):
            N.draw_indices(1, 0, 0, 10, 5, 1, block=bad)
    with pytest.raises(ValueError):
        N.draw_indices(1, 0, 0, 0, 5, 1, block=2)
    with pytest.raises(ValueError):
        N.draw_indices(1, 0, 0, 10, 0, 1, block=2)
    with pytest.raises(ValueError):
        N.draw_indices(1, 0, 0, 10, 5, 0, block=2)
    p = synth_genome(2, [30, 0], 3, 2, seed=1)
    with pytest.raises(ValueError, match="block"):
        N.resample(p, [(0, 5)], 2, 1, block=0)
    with pytest.raises(ValueError, match="empty"):
        N.resample(p, [(1, 5)], 2, 1, block=3)


def test_scan_pvalues_block_argument():
    import twoDSFS_class as T
    f = T.LikelihoodInference_jointSFS._null_block
    assert f(None) == 1 and f(1) == 1 and f(10) == 10 and f(np.int64(7)) == 7 and f("window") == (1 << 32) - 1
    for bad in (0, -3, 1 << 32, 2.5, "10", "windows", True):
        with pytest.raises(ValueError, match="block"):
            f(bad)
    p = synth_genome(1, [300], 18, 14, seed=2)
    dist = T.LikelihoodInference_jointSFS(None, None, pop1_size=18, pop2_size=14, distributed=True)
    with pytest.raises(NotImplementedError):
        dist.scan_pvalues(p, window_sizes=(8000,), block=10)


def test_cli_null_block_needs_replicates(capsys):
    from sfs2d import cli
    for argv in (["x.vcf", "x.txt", "--null-block", "10"], ["x.vcf", "x.txt", "--null-replicates", "9", "--null-block", "0"],
                 ["x.vcf", "x.txt", "--null-replicates", "9", "--null-block", "windows"]):
        with pytest.raises(SystemExit) as ei:
            cli.main(argv)
        assert ei.value.code == 2
        assert "--null-block" in capsys.readouterr().err


# ----------------------------------------------------------------------------- calibration on linked data (oracle only)

_CAL = {}


def _linked():
    """test_null_cpu's chromosome with its SNPs repeated in runs of geometric length, mean 5 (positions and
    annotations unchanged), the 400 windows of 50 SNPs against the per-chromosome background.  Computed once."""
    if not _CAL:
        p = synth_genome(1, [20000], 18, 14, seed=12345)
        runs = np.random.default_rng(12346).geometric(1 / 5, size=20000)
        idx = np.repeat(np.arange(20000), runs)[:20000]
        p = PackedSNPs(p.counts[idx], p.pos, p.chrom_off, list(p.chrom_names), p.ann_id, list(p.ann_names), p.pop1, p.pop2)
        cfg = O.Cfg(18, 14)
        bgs = O.chrom_backgrounds(p, cfg)
        wins, _ = O.snp_windows(p, 50)
        obs = U.oracle_records(p, [(c, i, b, e) for i, (c, _s, _e, b, e) in enumerate(wins)], cfg, lambda c: bgs[c])
        _CAL.update(p=p, cfg=cfg, bgs=bgs, obs=obs)
    return _CAL


def _block_p(block):
    cal = _linked()
    cls = N.size_classes(cal["obs"]["end"], "exact")
    assert len(cls) == 400 and np.all(cls == 50)
    q, wins = N.resample(cal["p"], [(0, 50)], 999, 0, block=block)
    null = U.oracle_records(q, wins, cal["cfg"], lambda c: cal["bgs"][c])
    pv = N.pvalues(cal["obs"], null, cls)["p_T2D"]
    assert not np.isnan(pv).any()
    return pv


def test_calibration_linked_data_window_blocks():
    """Blocks as long as the window on linked data: p_T2D is uniform.  Found (deterministic): KS distance
    0.0400, anti-conservative side sup (F_n(x) - x) 0.0225, mean p 0.505."""
    pv = _block_p(50)
    x = np.sort(pv)
    d, d_plus = U.ks_uniform(pv), float(np.max(np.arange(1, 401) / 400 - x))
    print(f"linked data, block 50: KS distance of p_T2D to U(0,1) {d:.4f}, anti-conservative side {d_plus:.4f}, mean p {pv.mean():.4f}")
    assert d < 1.95 / math.sqrt(400)


def test_calibration_linked_data_single_snp_null_fails():
    """Why the feature exists: against the single-SNP null (block 1) almost every window of the same linked
    data reads as significant.  Found: KS distance 0.9435, mean p 0.018."""
    pv = _block_p(1)
    d = U.ks_uniform(pv)
    print(f"linked data, block 1: KS distance of p_T2D to U(0,1) {d:.4f}, mean p {pv.mean():.4f}")
    assert d > 0.5
