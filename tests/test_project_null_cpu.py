"""The null of the projected scan on the host (sfs2d.projnull): the draws' twin, the records'
twin against a replicate worked by hand in Fractions, the p-value rule, the thin-slot count, the calibration of the
stratified null on heterogeneous missingness (and the failure of the unstratified one), and the argument errors of
the class and the CLI.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import projscan_util as PS
from sfs2d import _lib as L
from sfs2d import null as NL
from sfs2d import projnull as PN
from sfs2d import spectra as SP
from sfs2d.engine import ScanConfig
from sfs2d.pack import PackedSNPs, pack_counts

N1P, N2P = 18, 14
M = (24, 20)


def _cfg(**kw):
    return ScanConfig(n1p=N1P, n2p=N2P, **kw)


def _called(p):
    c = p.counts.astype(np.int64)
    return (c & 0xFF) + ((c >> 8) & 0xFF), ((c >> 16) & 0xFF) + (c >> 24)


# ------------------------------------------------------------------------------------------- draws

def test_draws_pinned():
    """One vector of the draws as literals: entry 100 of the 50-SNP windows, seed 7, the first 12 slots of 2
    replicates."""
    p = PS.genome(N1P, N2P, M)
    recs = PS.records(p, 50)
    assert (int(recs[100]["chrom"]), int(recs[100]["begin"]), int(recs[100]["end"])) == (9, 5157, 5207)
    d = PN.conditional_draws(p, recs, _cfg(), *M, [100], 2, 7)
    assert d[0].shape == (2, 50)
    assert d[0][:, :12].tolist() == [[-1, 11069, 7063, 8734, -1, 9724, 6942, 11644, 11216, -1, 10743, 9082],
                                     [-1, 6180, 10608, 13045, -1, 12582, 5380, 10174, 9735, -1, 9195, 8214]]


def test_draws_properties():
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg()
    recs = PS.records(p, 50)
    st = PN.strata(p, cfg, *M)
    nc1, nc2 = _called(p)
    # the pools: each chromosome's used SNPs, sorted by (n1c, n2c), ascending SNP index within a stratum
    for c, pool in enumerate(st.pool_idx):
        lo, hi = int(p.chrom_off[c]), int(p.chrom_off[c + 1])
        assert sorted(pool.tolist()) == (lo + np.nonzero(st.used[lo:hi])[0]).tolist()
        key = list(zip(nc1[pool].tolist(), nc2[pool].tolist(), pool.tolist()))
        assert key == sorted(key)
    u = np.nonzero(st.used)[0]
    assert (nc1[u] >= M[0]).all() and (nc2[u] >= M[1]).all() and (st.size[u] >= 1).all() and (st.size[~st.used] == 0).all()
    for k in u[::97].tolist():      # a SNP is in its own stratum, and the stratum is the pool's SNPs of its counts
        pool = st.pool_idx[int(st.chrom[k])]
        seg = pool[st.start[k]:st.start[k] + st.size[k]]
        assert k in seg.tolist()
        same = (nc1[pool] == nc1[k]) & (nc2[pool] == nc2[k])
        assert seg.tolist() == pool[same].tolist() == sorted(seg.tolist())
    rec = list(range(0, len(recs), 7))
    R = 5
    draws = PN.conditional_draws(p, recs, cfg, *M, rec, R, 3, st)
    alone = 0
    for s, d in zip(rec, draws):
        b, e = int(recs[s]["begin"]), int(recs[s]["end"])
        used = st.used[b:e]
        assert d.shape == (R, e - b) and (d[:, ~used] == -1).all() and (d[:, used] >= 0).all()      # an unused SNP draws nothing
        k = np.arange(b, e)[used]
        g = d[:, used]
        assert (st.chrom[g] == st.chrom[k][None, :]).all()
        assert (nc1[g] == nc1[k][None, :]).all() and (nc2[g] == nc2[k][None, :]).all() and st.used[g].all()   # in the stratum
        one = st.size[k] == 1
        assert (g[:, one] == k[one][None, :]).all()                    # alone in its stratum: draws itself
        alone += int(one.sum())
    assert alone > 0
    # splitting rec over calls, or another order, changes nothing per entry
    a = PN.conditional_draws(p, recs, cfg, *M, rec[:9], R, 3, st) + PN.conditional_draws(p, recs, cfg, *M, rec[9:], R, 3, st)
    back = PN.conditional_draws(p, recs, cfg, *M, rec[::-1], R, 3, st)[::-1]
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(draws, a, back))
    other = PN.conditional_draws(p, recs, cfg, *M, rec, R, 4, st)
    assert any(not np.array_equal(x, y) for x, y in zip(draws, other))
    # an EMPTY record has no slots
    dead = recs[:2].copy()
    dead["flags"][0] = L.W_EMPTY
    assert PN.conditional_draws(p, dead, cfg, *M, [0], 3, 0, st)[0].shape == (3, 0)


# ------------------------------------------------------------------------------------------- twin

def _hand(snps, bg_snps, m1, m2, fold):
    """(t2d, t1d_p1, t1d_p2) of a window of (r1, a1, r2, a2) SNPs against a background of such SNPs: grids in
    Fractions from the hypergeometric weights, the joint fold, the folded marginals, one logarithm per ratio."""
    def grid(rows):
        g = [[Fraction(0)] * (m2 + 1) for _ in range(m1 + 1)]
        for r1, a1, r2, a2 in rows:
            w1 = [Fraction(math.comb(a1, j) * math.comb(r1, m1 - j), math.comb(r1 + a1, m1)) for j in range(m1 + 1)]
            w2 = [Fraction(math.comb(a2, j) * math.comb(r2, m2 - j), math.comb(r2 + a2, m2)) for j in range(m2 + 1)]
            for i in range(m1 + 1):
                for j in range(m2 + 1):
                    g[i][j] += w1[i] * w2[j]
        if fold:
            for i in range(m1 + 1):
                for j in range(m2 + 1):
                    if 2 * (i + j) > m1 + m2:
                        g[m1 - i][m2 - j] += g[i][j]
                        g[i][j] = Fraction(0)
        return g

    def three(g):
        flat = [v for row in g for v in row][1:-1]
        s1 = [sum(row) for row in g]
        s2 = [sum(g[i][j] for i in range(m1 + 1)) for j in range(m2 + 1)]
        f1 = [s1[j] + s1[m1 - j] for j in range(1, m1 + 1) if 2 * j < m1]
        f2 = [s2[j] + s2[m2 - j] for j in range(1, m2 + 1) if 2 * j < m2]
        return flat, f1, f2
    out = []
    for x, b in zip(three(grid(snps)), three(grid(bg_snps))):
        N, B = sum(x), sum(b)
        out.append(2.0 * math.fsum(float(v) * (math.log(v / N) - math.log(w / B)) for v, w in zip(x, b) if v > 0))
    return out


def test_twin_against_a_replicate_by_hand():
    """One chromosome of 9 SNPs at (7, 5), three windows of 3: the twin's records (exact and float weights) against
    the replicate of window 1 worked in Fractions from the drawn SNPs."""
    m1, m2 = 7, 5
    rows = [(5, 4, 3, 4), (7, 1, 4, 2), (4, 6, 2, 6), (3, 6, 6, 1), (2, 7, 7, 1), (2, 6, 1, 5), (2, 8, 2, 5), (8, 1, 2, 5),
            (9, 0, 7, 0)]      # called counts (9, 7) x 3, (8, 6) x 2, three alone; the last one is no member
    cols = [np.array(c, np.int64) for c in zip(*rows)]
    p = PackedSNPs(pack_counts(*cols), np.arange(1, 10) * 100, np.array([0, 9]), ["c"], None)
    for fold in (True, False):
        cfg = ScanConfig(n1p=5, n2p=4, fold=fold, window_mode=L.WINDOW_SNPS, window=3)
        recs = PS.records(p, 3)
        st = PN.strata(p, cfg, m1, m2)
        assert st.used.tolist() == [True] * 8 + [False] and st.size[:8].tolist() == [3, 2, 1, 3, 1, 2, 1, 3]
        draws = PN.conditional_draws(p, recs, cfg, m1, m2, [1, 2], 4, 11, st)
        assert (draws[1][:, 2] == -1).all() and {int(v) for v in draws[0][:, 0]} <= {0, 3, 7}
        members = [rows[k] for k in range(9) if st.member[k]]
        for exact in (True, False):
            tw, thin = PN.project_null_np(p, recs, cfg, m1, m2, [1, 2], 4, 11, exact=exact)
            assert thin.tolist() == [3, 2] and tw["n_used"].tolist() == [3] * 4 + [2] * 4 and not tw["n_dropped"].any()
            for t in range(2):
                for r in range(4):
                    want = _hand([rows[k] for k in draws[t][r] if k >= 0], members, m1, m2, fold)
                    got = [float(tw[f][t * 4 + r]) for f in ("t2d", "t1d_p1", "t1d_p2")]
                    assert all(abs(g - w) <= 1e-12 * max(1.0, abs(w)) for g, w in zip(got, want)), (fold, exact, t, r, got, want)


def test_all_dropped_window_is_nan_and_none():
    m = (7, 5)
    p = PS.genome(N1P, N2P, m)
    cfg = _cfg(window_mode=L.WINDOW_SNPS, window=3)
    recs = PS.records(p, 3)
    i = int(np.nonzero(recs["begin"] == int(p.chrom_off[-2]) + PS.ALL_DROPPED)[0][0])
    for exact in (True, False):
        tw, thin = PN.project_null_np(p, recs, cfg, *m, [i, i + 1], 3, 0, exact=exact)
        assert all(np.isnan(tw[f][:3]).all() for f in ("t2d", "t1d_p1", "t1d_p2")) and thin[0] == 0
        assert tw["n_used"][:3].tolist() == [0] * 3 and tw["n_dropped"][:3].tolist() == [3] * 3
        assert np.isfinite(tw["t2d"][3:]).all()
    obs = SP.project_scan_np(p, recs[[i, i + 1]], cfg, *m)
    pv = PN.project_pvalues(obs, tw, 3)
    assert all(math.isnan(pv[k][0]) and 0 < pv[k][1] <= 1 for k in PN.PROJ_P_KEYS)
    rows = SP.project_scan_rows(recs[[i, i + 1]], obs, ["a", "b"])
    PN.add_pvalue_columns(rows, ["a", "b"], pv, thin)
    assert all(rows["a"][k] is None for k in PN.PROJ_P_KEYS) and rows["a"]["n_thin"] == 0
    assert list(rows["b"])[-7:] == PN.PROJNULL_COLUMNS and rows["b"]["p_T2D_proj"] == pv["p_T2D_proj"][1]


def _stat(t2, ta, tb, flags=0):
    a = np.zeros(len(t2), L.PROJSTAT_DTYPE)
    a["t2d"], a["t1d_p1"], a["t1d_p2"], a["flags"] = t2, ta, tb, flags
    return a


def test_pvalue_rule():
    inf, nan = math.inf, math.nan
    obs = _stat([10.0, inf, nan, 10.0, 5.0], [1.0, 1.0, 1.0, inf, 1.0], [2.0, 2.0, 2.0, 2.0, 2.0], [0, 0, 0, 0, L.W_EMPTY])
    R = 4
    t2 = [10.0 - 5e-9, 10.0 - 2e-8, nan, inf]      # a tie within the slack, one outside it, a NaN, +inf
    null = _stat(t2 * 5, [1.0, 0.5, 1.0, inf] * 5, [2.0] * 20)
    pv = PN.project_pvalues(obs, null, R)
    p2 = pv["p_T2D_proj"]
    assert p2[0] == (1 + 2) / 5 and p2[1] == (1 + 1) / 5 and math.isnan(p2[2]) and math.isnan(p2[4])      # inf: its own threshold
    assert pv["p_T1D_pop1_proj"][:3].tolist() == [(1 + 3) / 5] * 3 and pv["p_T1D_pop1_proj"][3] == (1 + 1) / 5
    # derived terms: formed per record; inf - inf and NaN operands are None / never count
    d = pv["p_new_term_pop1_proj"]
    # null t2 - ta: [9 - 5e-9, 9.5 - 2e-8, NaN, inf - inf = NaN] against 9 (two count) and against 10 - inf = -inf,
    # its own threshold (the same two)
    assert d[0] == (1 + 2) / 5 and math.isnan(d[2]) and d[3] == (1 + 2) / 5 and math.isnan(pv["p_T2D_diff_proj"][4])
    both = _stat([inf], [inf], [1.0])      # inf - inf: None, as project_scan_rows has it
    assert math.isnan(PN.project_pvalues(both, null[:4], R)["p_new_term_pop1_proj"][0])
    with pytest.raises(ValueError):
        PN.project_pvalues(obs, null[:-1], R)


def test_n_thin_counts_small_strata():
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg()
    recs = PS.records(p, 50)
    st = PN.strata(p, cfg, *M)
    nc1, nc2 = _called(p)
    _, thin = PN.project_null_np(p, recs, cfg, *M, [0, 5, 100, 277], 1, 0, st=st)
    for t, s in enumerate((0, 5, 100, 277)):
        b, e, c = int(recs[s]["begin"]), int(recs[s]["end"]), int(recs[s]["chrom"])
        lo, hi = int(p.chrom_off[c]), int(p.chrom_off[c + 1])
        want = 0
        for k in range(b, e):
            if st.used[k]:
                peers = int((st.used[lo:hi] & (nc1[lo:hi] == nc1[k]) & (nc2[lo:hi] == nc2[k])).sum())
                want += peers < L.PNULL_THIN
        assert thin[t] == want
    assert thin.sum() > 0 and (thin <= 50).all()


# ------------------------------------------------------------------------------------------- calibration

def _ks(x):
    x = np.sort(np.asarray(x, np.float64))
    n = len(x)
    i = np.arange(1, n + 1)
    return float(max((i / n - x).max(), (x - (i - 1) / n).max()))


def test_calibration_stratified_null_is_uniform_unstratified_is_not():
    """No signal in the data, alleles missing at 2 % in even 50-SNP windows and 25 % in odd ones: p_T2D_proj of the
    stratified null is uniform (Kolmogorov-Smirnov distance below the 0.1 % critical values 0.0975 for 400 windows and
    0.138 for each half of 200), of section 14's design applied to the projected statistic -- n_used draws from the
    chromosome's used SNPs whatever their called counts -- it is not (KS > 0.25).  Found: stratified 0.045 / 0.075 /
    0.060 (mean p 0.527 / 0.497), unstratified 0.365 (mean p 0.942 / 0.035), 0.53 % of used slots thin."""
    from sfs2d.synth import synth_genome
    g = synth_genome(1, [20000], N1P, N2P, seed=12345, n_ann=3)
    c = g.counts.astype(np.int64)
    alt1, alt2 = (c >> 8) & 0xFF, c >> 24
    # (every SNP taken as fully called: ref = 2 pop - alt, the generator's own missing alleles put back)
    rng = np.random.default_rng(99)
    rate = np.where((np.arange(g.n) // 50) % 2 == 0, 0.02, 0.25)
    cols = []
    for alt, pop in ((alt1, N1P), (alt2, N2P)):
        a = rng.binomial(alt, 1 - rate)
        r = rng.binomial(2 * pop - alt, 1 - rate)
        cols += [r, a]
    p = PackedSNPs(pack_counts(*cols), g.pos, g.chrom_off, g.chrom_names, g.ann_id, g.ann_names)
    cfg = _cfg(window_mode=L.WINDOW_SNPS, window=50)
    recs = PS.records(p, 50)
    R = 199
    assert len(recs) == 400
    st = PN.strata(p, cfg, *M)
    null, thin = PN.project_null_np(p, recs, cfg, *M, None, R, 0, st=st)
    # the observed windows through the same evaluation: the "replicate" in which every used SNP draws itself
    own = [np.where(st.used[b:e], np.arange(b, e), -1)[None, :] for b, e in zip(recs["begin"].tolist(), recs["end"].tolist())]
    obs, _ = PN.project_null_np(p, recs, cfg, *M, None, 1, 0, draws=own, st=st)
    pv = PN.project_pvalues(obs, null, R)["p_T2D_proj"]
    ks = (_ks(pv), _ks(pv[0::2]), _ks(pv[1::2]))
    share = thin.sum() / obs["n_used"].sum()
    # the unstratified control: NL.draw_indices over the chromosome's used SNPs, m = n_used, the same evaluation
    pool = np.nonzero(st.used)[0]
    ctl = []
    for s, (b, e) in enumerate(zip(recs["begin"].tolist(), recs["end"].tolist())):
        full = np.full((R, e - b), -1, np.int64)
        full[:, st.used[b:e]] = pool[NL.draw_indices(0, 0, 0, len(pool), int(obs["n_used"][s]), R)]
        ctl.append(full)
    null_c, _ = PN.project_null_np(p, recs, cfg, *M, None, R, 0, draws=ctl, st=st)
    pc = PN.project_pvalues(obs, null_c, R)["p_T2D_proj"]
    print(f"stratified KS {ks[0]:.4f} / {ks[1]:.4f} / {ks[2]:.4f} (mean p {pv[0::2].mean():.3f} / {pv[1::2].mean():.3f}), "
          f"unstratified KS {_ks(pc):.4f} (mean p {pc[0::2].mean():.3f} / {pc[1::2].mean():.3f}), thin share {share:.4%}")
    assert share < 0.02
    assert ks[0] < 0.0975 and ks[1] < 0.138 and ks[2] < 0.138
    assert _ks(pc) > 0.25


# ------------------------------------------------------------------------------------------- class, CLI, exports

def test_class_argument_errors():
    import twoDSFS_class as T
    p = PS.genome(N1P, N2P, M)
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=N1P, pop2_size=N2P)
    with pytest.raises(NotImplementedError):
        obj.projected_scan(p, M, window_size=20000, background_chromosome=p.chrom_names[9], replicates=9)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            obj.projected_scan(p, M, window_size=20000, replicates=bad)
    dist = T.LikelihoodInference_jointSFS(None, None, pop1_size=N1P, pop2_size=N2P, distributed=True)
    with pytest.raises(NotImplementedError):
        dist.projected_scan(p, M, window_size=20000, replicates=9)


@pytest.mark.parametrize("extra", [["--project-null", "9"], ["--project-scan", "16,14", "--project-null", "0"],
                                   ["--project-scan", "16,14", "--project-null", "-3"],
                                   ["--project-scan", "16,14", "--project-null", "many"],
                                   ["--project-scan", "16,14", "--project-null", "2.5"]])
def test_cli_argument_errors(extra, capsys):
    from sfs2d import cli
    with pytest.raises(SystemExit) as ei:
        cli.main(["no.vcf", "no.popmap", "--pop1-size", "11", "--pop2-size", "11"] + extra)
    assert ei.value.code == 2 and "--project-null" in capsys.readouterr().err


def test_exports():
    import os
    assert {"sfs2d_plan_project_null", "sfs2d_plan_project_null_read"} <= set(L.EXPORTS)
    assert L.PNULL_THIN == 8
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "sfs2d.h")) as fh:
        h = fh.read()
    assert "int sfs2d_plan_project_null(" in h and "int sfs2d_plan_project_null_read(" in h
    assert "#define SFS2D_PNULL_THIN 8" in h and "#define SFS2D_ABI_VERSION 2" in h
    for name in PN.__all__:
        assert hasattr(PN, name)
    assert PN.PROJNULL_COLUMNS == ["p_T2D_proj", "p_T1D_pop1_proj", "p_T1D_pop2_proj", "p_new_term_pop1_proj",
                                   "p_new_term_pop2_proj", "p_T2D_diff_proj", "n_thin"]
