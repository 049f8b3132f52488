"""Bootstrap null, host side (sfs2d.null): size classes, the host twin of the
device's draws, the p-value definition, and the calibration of the definition itself with the oracle
standing in for the device (no GPU)."""
import math

import numpy as np
import pytest

import null_util as U
from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import null as N
from sfs2d.pack import PackedSNPs, pack_counts
from sfs2d.synth import _philox, synth_genome


# ----------------------------------------------------------------------------- size classes

def test_default_grid_first_terms():
    # ceil(g * 2**(1/8)) <= g + 1 while g * 0.0905 <= 1, i.e. g <= 11: steps of one up to 12, then geometric
    # (12 * 1.0905 = 13.09 -> 14, 14 -> 15.27 -> 16, ..., 24 -> 26.17 -> 27, 27 -> 29.44 -> 30, ...)
    assert N.default_grid(101).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 18, 20, 22, 24, 27, 30, 33, 36,
                                            40, 44, 48, 53, 58, 64, 70, 77, 84, 92, 101]
    g = N.default_grid(100000)
    assert g[-1] >= 100000 > g[-2]
    assert np.all(g[1:] == np.maximum(g[:-1] + 1, np.ceil(g[:-1] * 2.0 ** 0.125).astype(np.int64)))


def test_size_classes_map_up_within_nine_percent():
    ms = np.arange(1, 5000)
    c = N.size_classes(ms)
    assert np.all(c >= ms)
    assert np.all((c - ms) / ms <= 2.0 ** 0.125 - 1.0)            # the 9 % bound
    assert np.all(np.isin(c, N.default_grid(5000)))
    g = N.default_grid(5000)
    assert np.all(c == g[np.searchsorted(g, ms)])                   # the smallest class >= m
    assert N.size_classes([50, 53, 54]).tolist() == [53, 53, 58]
    assert N.size_classes([]).size == 0


def test_size_classes_exact_and_list():
    assert N.size_classes([7, 50, 50, 358], "exact").tolist() == [7, 50, 50, 358]
    assert N.size_classes([7, 50, 358], [10, 100, 400]).tolist() == [10, 100, 400]
    assert N.size_classes([10, 11], [10, 100]).tolist() == [10, 100]
    with pytest.raises(ValueError, match="below the largest window"):
        N.size_classes([7, 401], [10, 100, 400])
    with pytest.raises(ValueError):
        N.size_classes([7], [100, 10])
    with pytest.raises(ValueError):
        N.size_classes([0])
    with pytest.raises(ValueError):
        N.size_classes([5], "nearest")


# ----------------------------------------------------------------------------- draws

def test_draw_indices_range_and_degenerate_pool():
    d = N.draw_indices(3, 1, 1000, 77, 129, 11)
    assert d.shape == (11, 129) and d.dtype == np.int64
    assert d.min() >= 1000 and d.max() < 1077
    assert len(np.unique(d)) == 77                                   # 1,419 draws reach all 77 SNPs
    assert np.all(N.draw_indices(3, 1, 42, 1, 9, 5) == 42)           # n = 1: lo everywhere
    big = N.draw_indices(9, -1, 0, (1 << 32) - 1, 64, 4)             # the largest pool: no overflow in mulhi64
    assert big.min() >= 0 and big.max() < (1 << 32) - 1 and big.max() > 1 << 31


def test_draws_depend_on_the_task_alone():
    p = synth_genome(3, [300, 5, 120], 3, 2, seed=1)
    tasks = [(0, 7), (2, 64), (0, 8), (2, 7)]
    q, wins = N.resample(p, tasks, 6, seed=11)
    assert len(wins) == 24 and q.n == 6 * (7 + 64 + 8 + 7)
    for t, (pool, m) in enumerate(tasks):
        lo, n = N.pool_range(p, pool)
        alone = N.draw_indices(11, pool, lo, n, m, 6)
        q1, w1 = N.resample(p, [(pool, m)], 6, seed=11)               # the task on its own
        for r in range(6):
            c, rr, b, e = wins[t * 6 + r]
            assert (c, rr, e - b) == (pool, r, m)
            assert np.array_equal(q.counts[b:e], p.counts[alone[r]]) and np.array_equal(q.pos[b:e], p.pos[alone[r]])
            assert np.array_equal(q.counts[b:e], q1.counts[w1[r][2]:w1[r][3]])
    # replicate r is the same whether 6 or 2 replicates are asked for
    assert np.array_equal(N.draw_indices(11, 0, 0, 300, 7, 6)[:2], N.draw_indices(11, 0, 0, 300, 7, 2))
    # the class is in the counter: the first 7 draws of m = 8 are not the draws of m = 7; nor are another
    # pool's, another replicate's or another seed's
    a = N.draw_indices(11, 0, 0, 300, 7, 6)
    assert not np.array_equal(a, N.draw_indices(11, 0, 0, 300, 8, 6)[:, :7])
    assert not np.array_equal(a, N.draw_indices(11, 1, 0, 300, 7, 6))
    assert not np.array_equal(a, N.draw_indices(12, 0, 0, 300, 7, 6))
    assert not np.array_equal(a, N.draw_indices(11 + (1 << 32), 0, 0, 300, 7, 6))   # the seed's high word is key 1
    assert not np.array_equal(a[0], a[1])
    assert np.array_equal(N.draw_indices(5, -1, 0, 425, 9, 3), N.draw_indices(5, -1, 0, 425, 9, 3))


def test_pinned_draw_vector():
    """seed 1, pool 0, n = 1000, m = 5, r = 0.  The Philox words were computed once with synth._philox for
    counters (0, 0, 5, 1), (1, 0, 5, 1), (2, 0, 5, 1) and key (1, 0):
      j = 0, 1: c = (3756316396, 3743554222, 2056008249, 160431284)
      j = 2, 3: c = (253649424, 3153771683, 2354235224, 2628740830)
      j = 4:    c = (1616236942, 2038089843, ...)
    and the index is floor((lo32 + hi32 * 2**32) * 1000 / 2**64), written here as literals."""
    c = _philox(np.array([0, 1, 2]), 0, 5, 1, 1, 0)
    assert [int(x[0]) for x in c] == [3756316396, 3743554222, 2056008249, 160431284]
    assert [int(x[1]) for x in c] == [253649424, 3153771683, 2354235224, 2628740830]
    assert [int(x[2]) for x in c[:2]] == [1616236942, 2038089843]
    for lo32, hi32, want in ((3756316396, 3743554222, 871), (2056008249, 160431284, 37), (253649424, 3153771683, 734),
                             (2354235224, 2628740830, 612), (1616236942, 2038089843, 474)):
        assert ((lo32 + (hi32 << 32)) * 1000) >> 64 == want
    assert N.draw_indices(1, 0, 0, 1000, 5, 1).tolist() == [[871, 37, 734, 612, 474]]
    assert N.draw_indices(1, 0, 250, 1000, 5, 1).tolist() == [[1121, 287, 984, 862, 724]]


# ----------------------------------------------------------------------------- p-values on hand-made records

def _recs(t2, ta=None, tb=None, chrom=0, m=10, n=(1, 1, 1), flags=0):
    k = len(t2)
    r = np.zeros(k, L.WINDOW_DTYPE)
    r["chrom"], r["end"], r["flags"] = chrom, m, flags
    r["n2"], r["n1a"], r["n1b"] = n
    r["t2d"] = t2
    r["t1d_p1"] = np.zeros(k) if ta is None else ta
    r["t1d_p2"] = np.zeros(k) if tb is None else tb
    return r


def test_pvalue_rule():
    null = _recs(np.arange(1.0, 10.0))                                 # R = 9: T* = 1 .. 9
    obs = _recs([0.5, 1.0, 5.5, 9.0, 9.5])
    pv = N.pvalues(obs, null, [10] * 5)
    assert pv["p_T2D"].tolist() == [(1 + 9) / 10, (1 + 9) / 10, (1 + 4) / 10, (1 + 1) / 10, (1 + 0) / 10]
    assert set(pv) == set(N.P_KEYS) == {"p_T2D", "p_T1D_pop1", "p_T1D_pop2", "p_new_term_pop1", "p_new_term_pop2",
                                        "p_T2D_diff"}


def test_pvalue_slack_breaks_ties_toward_counting():
    t = 37.25
    null = _recs([t * (1 - 5e-11), t * (1 - 5e-9), t, 0.3 - 5e-10, 0.3 - 5e-9])
    pv = N.pvalues(_recs([t, 0.3]), null, [10, 10])
    # T = 37.25: the planted tie 5e-11 below counts, 5e-9 below does not; 0.3: the slack is absolute below 1
    assert pv["p_T2D"].tolist() == [(1 + 2) / 6, (1 + 4) / 6]


def test_pvalue_none_rules():
    null = _recs([1.0, 2.0, 3.0, 4.0])
    null["n2"][1] = 0                                                  # an invalid null value: N == 0 ...
    null["flags"][3] = L.W_BG2_ZERO                                    # ... or an empty background
    null["t2d"][[1, 3]] = 100.0                                        # (whatever the field holds)
    obs = _recs([0.0, 0.0, 0.0])
    obs["n2"][1] = 0
    obs["flags"][2] = L.W_BG2_ZERO
    pv = N.pvalues(obs, null, [10] * 3)
    assert pv["p_T2D"][0] == (1 + 2) / 5                               # invalid nulls stay in the denominator
    assert np.isnan(pv["p_T2D"][1]) and np.isnan(pv["p_T2D"][2])       # observed None -> None
    assert pv["p_T1D_pop1"][1] == 1.0 and np.isnan(pv["p_new_term_pop1"][1]) and np.isnan(pv["p_T2D_diff"][1])
    # inf counts against inf, NaN against nothing
    null = _recs([1.0, math.inf, math.nan])
    pv = N.pvalues(_recs([math.inf, math.nan, 2.0]), null, [10] * 3)
    assert pv["p_T2D"].tolist() == [(1 + 1) / 4, (1 + 0) / 4, (1 + 1) / 4]


def test_pvalue_derived_terms_from_own_values_and_by_task():
    null = np.concatenate([_recs([10.0, 10.0, 10.0], [1.0, 5.0, 9.0], [1.0, 1.0, 1.0], chrom=0, m=10),
                           _recs([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], chrom=1, m=10),
                           _recs([9.0, 9.0, 9.0], chrom=0, m=12)])
    null["n1a"][0] = 0                                                 # pop 1 invalid in replicate 0
    obs = _recs([10.0], [4.0], [2.0])
    pv = N.pvalues(obs, null, [10])
    # new_term_pop1 = 6: replicates 1 (5) and 2 (1) valid, replicate 0 invalid; 5 < 6, 1 < 6
    assert pv["p_new_term_pop1"][0] == (1 + 0) / 4
    assert pv["p_new_term_pop2"][0] == (1 + 3) / 4                     # 8 against 9, 9, 9
    assert pv["p_T2D_diff"][0] == (1 + 1) / 4                          # 7 against (invalid), 7, 5
    assert N.pvalues(obs, null, [12])["p_T2D"][0] == (1 + 0) / 4       # the class picks the task
    assert N.pvalues(obs, null, [10], pools=[1])["p_T2D"][0] == (1 + 0) / 4   # and so does the pool
    with pytest.raises(ValueError):
        N.pvalues(obs, null, [11])


def test_pvalues_device_path_equals_host_on_cpu_tensors():
    """pvalues_device (torch sort / searchsorted) against pvalues, on a CPU tensor: invalid records, ties,
    inf and NaN values, several tasks, the all-SNPs pool."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)

    def mk(n, chrom, m):
        r = _recs(rng.integers(0, 6, n).astype(float), rng.integers(0, 6, n).astype(float), rng.integers(0, 5, n).astype(float),
                  chrom=chrom & 0xFFFFFFFF, m=m, n=(rng.integers(0, 3, n), rng.integers(0, 3, n), rng.integers(0, 3, n)),
                  flags=rng.integers(0, 2, n) * rng.integers(0, 8, n))
        r["t2d"][rng.random(n) < 0.1] = math.inf
        r["t1d_p1"][rng.random(n) < 0.1] = math.inf
        r["t2d"][rng.random(n) < 0.05] = math.nan
        return r
    tasks, R = [(0, 4), (-1, 4), (1, 8)], 50
    null = np.concatenate([mk(R, c, m) for c, m in tasks])
    obs = np.concatenate([mk(40, c, m) for c, m in reversed(tasks)])
    a = N.pvalues(obs, null, obs["end"])
    b = N.pvalues_device(obs, obs["end"], torch.from_numpy(null.view(np.uint8).copy()), tasks, R)
    for k in N.P_KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.isnan(a[k]).any() and (a[k] > 1 / (R + 1)).any()


# ----------------------------------------------------------------------------- calibration and power (oracle only)

_CAL = {}


def _calibration():
    """One chromosome of 20,000 i.i.d. SNPs, (18, 14), per-chromosome background, 400 windows of 50 SNPs;
    R = 999 replicates per size class from resample + oracle.window_records.  Computed once."""
    if not _CAL:
        p = synth_genome(1, [20000], 18, 14, seed=12345)
        cfg = O.Cfg(18, 14)
        bgs = O.chrom_backgrounds(p, cfg)
        wins, _ = O.snp_windows(p, 50)
        obs = U.oracle_records(p, [(c, i, b, e) for i, (c, _s, _e, b, e) in enumerate(wins)], cfg, lambda c: bgs[c])
        _CAL.update(p=p, cfg=cfg, bgs=bgs, obs=obs)
    return _CAL


def _null_p(cal, sizes):
    cls = N.size_classes(cal["obs"]["end"], sizes)
    tasks = sorted(set((0, int(m)) for m in cls))
    assert len(tasks) == 1                                              # 400 windows, one class
    null, _, _ = U.null_twin(cal["p"], tasks, 999, 0, cal["cfg"], lambda c: cal["bgs"][c])
    return N.pvalues(cal["obs"], null, cls)["p_T2D"], tasks[0][1]


def test_calibration_exact_class():
    """The definition itself: the null of a 50-SNP window is 50 draws (sizes="exact").  The synthetic SNPs
    are i.i.d. along the chromosome, so p_T2D of the 400 windows is uniform: its Kolmogorov-Smirnov distance
    to U(0, 1) must be below 1.95 / sqrt(400) = 0.0975, the 0.1 % critical value.
    Found (seed 12345, null seed 0, deterministic): 0.0390."""
    pv, m = _null_p(_calibration(), "exact")
    assert m == 50 and len(pv) == 400 and not np.isnan(pv).any()
    d = U.ks_uniform(pv)
    print(f"KS distance of p_T2D to U(0,1), class 50: {d:.4f}")
    assert d < 1.95 / math.sqrt(400)


def test_calibration_default_class_is_conservative():
    """The same windows through the default size grid, which rounds 50 up to the class 53.  Found: the
    two-sided distance is 0.1460, above the 0.0975 critical value -- a 6 % larger window has a visibly larger
    null T, so the rounding is NOT negligible for calibration (DESIGN.md section 14 says so and points to
    sizes="exact").  What the rounding is meant to guarantee is the direction: p-values can only grow.  The
    one-sided distance in the anti-conservative direction, sup (F_n(x) - x), must stay below the same
    0.0975 (found: 0.0020), and the mean p-value must not fall below the exact class's (found: 0.5092 ->
    0.5810)."""
    cal = _calibration()
    pv, m = _null_p(cal, None)
    assert m == 53
    x = np.sort(pv)
    i = np.arange(1, 401)
    d_plus, d_two = float(np.max(i / 400 - x)), U.ks_uniform(pv)
    exact, _ = _null_p(cal, "exact")
    print(f"class 53: two-sided KS {d_two:.4f}, anti-conservative side {d_plus:.4f}, mean p {exact.mean():.4f} -> {pv.mean():.4f}")
    assert d_plus < 1.95 / math.sqrt(400)
    assert pv.mean() >= exact.mean()


def test_power_planted_window():
    """50 consecutive SNPs overwritten with (alt1, alt2) = (2 n1, 0) / (0, 2 n2) alternating: no replicate
    window reaches that window's T2D, so its p_T2D is exactly 1 / (R + 1)."""
    cal = _calibration()
    p, cfg = cal["p"], cal["cfg"]
    n1, n2 = 2 * cfg.n1p, 2 * cfg.n2p
    even = np.arange(50) % 2 == 0
    counts = p.counts.copy()
    counts[5000:5050] = pack_counts(np.where(even, 0, n1), np.where(even, n1, 0), np.where(even, n2, 0), np.where(even, 0, n2))
    q = PackedSNPs(counts, p.pos, p.chrom_off, list(p.chrom_names), p.ann_id, list(p.ann_names), p.pop1, p.pop2)
    bgs = O.chrom_backgrounds(q, cfg)
    obs = U.oracle_records(q, [(0, 100, 5000, 5050)], cfg, lambda c: bgs[c])
    null, _, _ = U.null_twin(q, [(0, 50)], 999, 0, cfg, lambda c: bgs[c])
    pv = N.pvalues(obs, null, N.size_classes(obs["end"], "exact"))
    assert pv["p_T2D"][0] == 1.0 / 1000.0
    assert float(obs["t2d"][0]) > 2.0 * float(null["t2d"].max())
