"""The projected scan without a GPU: the numpy twin sfs2d.spectra.project_scan_np against
literals worked by hand and against the oracle, the +inf / NaN / None rules, project_scan_rows, the class's and the
CLI's argument errors, the exports, and the properties of the fixtures the GPU tests use (tests/projscan_util.py)."""
import math
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

import project_util as PU
import projscan_util as PS
from sfs2d import _lib as L
from sfs2d import spectra as SP

N1P, N2P = 18, 14


def _tiny():
    from sfs2d.pack import PackedSNPs, pack_counts
    s = np.array([(3, 1, 2, 2), (1, 2, 3, 1), (0, 4, 1, 3), (2, 2, 2, 2), (3, 1, 4, 0), (4, 0, 3, 1)])
    p = PackedSNPs(pack_counts(s[:, 0], s[:, 1], s[:, 2], s[:, 3]), np.arange(1, 7, dtype=np.uint32) * 10,
                   np.array([0, 6]), ["c1"], np.zeros(6, np.uint16), ["x"])
    recs = np.zeros(2, L.WINDOW_DTYPE)
    recs["begin"], recs["end"] = [0, 3], [3, 6]
    return p, recs


def _t(x, b):
    """2 sum x_k (ln(x_k / N) - ln(b_k / B)) of the listed Fractions."""
    N, B = sum(x), sum(b)
    return 2 * math.fsum(float(xk) * (math.log(xk / N) - math.log(bk / B)) for xk, bk in zip(x, b) if xk)


def test_twin_against_hand_worked_literals():
    """Two populations of 2 diploids (4 alleles each), one chromosome of six SNPs (ref1, alt1, ref2, alt2):
        S1 (3, 1, 2, 2)   S2 (1, 2, 3, 1): one allele of population 1 missing   S3 (0, 4, 1, 3)
        S4 (2, 2, 2, 2)   S5 (3, 1, 4, 0)   S6 (4, 0, 3, 1)
    The window is S1 .. S3, the background all six.  Weights h(j; n, a, m) = C(a, j) C(n - a, m - j) / C(n, m):
        m = 2:  (4, 0) [1, 0, 0]  (4, 1) [1/2, 1/2, 0]  (4, 2) [1/6, 2/3, 1/6]  (4, 3) [0, 1/2, 1/2]  (4, 4) [0, 0, 1]
                (3, 2) [0, 2/3, 1/3]
        m = 3:  (4, 0) [1, 0, 0, 0]  (4, 1) [1/4, 3/4, 0, 0]  (4, 2) [0, 1/2, 1/2, 0]  (4, 4) [0, 0, 0, 1]
                (3, 2) [0, 0, 1, 0]   (n = m: the indicator of a)
    (2, 2), unfolded: window = S1 [1/2, 1/2, 0] x [1/6, 2/3, 1/6] + S2 [0, 2/3, 1/3] x [1/2, 1/2, 0] + S3 [0, 0, 1] x
    [0, 1/2, 1/2] = [[1/12, 1/3, 1/12], [5/12, 2/3, 1/12], [1/6, 2/3, 1/2]]; inner bins (all but the first and the
    last) N = 3 - 1/12 - 1/2 = 29/12.  Background: [[10/9, 17/18, 1/9], [37/36, 10/9, 7/36], [7/36, 7/9, 19/36]], B =
    6 - 10/9 - 19/36 = 157/36.  Folded (bins with j1 + j2 > 2 go to (2 - j1, 2 - j2), the anti-diagonal stays): window
    [[7/12, 1, 1/12], [1/2, 2/3, 0], [1/6, 0, 0]], background [[59/36, 31/18, 1/9], [11/9, 10/9, 0], [7/36, 0, 0]]: the
    first bin gained the last one's, N and B are unchanged.  m = 2 has no inner 1D bin (1 <= j, 2 j < 2): T1D is NaN.
    (3, 2): S2 has n1 = 3 = m1, so its population-1 weights are the indicator of bin 2.  Unfolded window [[1/24, 1/6,
    1/24], [1/8, 1/2, 1/8], [1/2, 1/2, 0], [0, 1/2, 1/2]], N = 3 - 1/24 - 1/2 = 59/24; background [[19/24, 2/3, 1/24],
    [23/24, 5/6, 5/24], [7/12, 5/6, 1/12], [0, 1/2, 1/2]], B = 6 - 19/24 - 1/2 = 113/24.  Folded (2 (j1 + j2) > 5):
    window [[13/24, 2/3, 1/24], [1/8, 1, 0], [5/8, 0, 0], [0, 0, 0]], background [[31/24, 7/6, 1/24], [25/24, 5/3, 0],
    [19/24, 0, 0], [0, 0, 0]].  The population-1 marginal folded min(j, 3 - j) has the one inner bin j = 1, rows 1 and
    2: window 7/4, background 7/2 -- one bin against one bin: T1D_pop1 = 2 x 7/4 x (ln 1 - ln 1) = 0; population 2
    (m = 2) has none: NaN."""
    p, recs = _tiny()
    cases = {
        ((2, 2), False): ([F(1, 3), F(1, 12), F(5, 12), F(2, 3), F(1, 12), F(1, 6), F(2, 3)],
                          [F(17, 18), F(1, 9), F(37, 36), F(10, 9), F(7, 36), F(7, 36), F(7, 9)], F(29, 12)),
        ((2, 2), True): ([F(1), F(1, 12), F(1, 2), F(2, 3), F(0), F(1, 6), F(0)],
                         [F(31, 18), F(1, 9), F(11, 9), F(10, 9), F(0), F(7, 36), F(0)], F(29, 12)),
        ((3, 2), False): ([F(1, 6), F(1, 24), F(1, 8), F(1, 2), F(1, 8), F(1, 2), F(1, 2), F(0), F(0), F(1, 2)],
                          [F(2, 3), F(1, 24), F(23, 24), F(5, 6), F(5, 24), F(7, 12), F(5, 6), F(1, 12), F(0), F(1, 2)],
                          F(59, 24)),
        ((3, 2), True): ([F(2, 3), F(1, 24), F(1, 8), F(1), F(0), F(5, 8), F(0), F(0), F(0), F(0)],
                         [F(7, 6), F(1, 24), F(25, 24), F(5, 3), F(0), F(19, 24), F(0), F(0), F(0), F(0)], F(59, 24)),
    }
    for (m, fold), (x, b, N) in cases.items():
        assert sum(x) == N
        want = _t(x, b)
        for exact in (True, False):
            got = SP.project_scan_np(p, recs, PU.Cfg(2, 2, fold=fold), *m, exact=exact)[0]
            assert got["t2d"] == pytest.approx(want, rel=1e-13) and want > 0.05, (m, fold, exact)
            assert got["n2"] == float(N) and (got["n_used"], got["n_dropped"], got["flags"]) == (3, 0, 0)
            assert math.isnan(got["t1d_p2"]) and got["n1b"] == 0
            if m == (2, 2):
                assert math.isnan(got["t1d_p1"]) and got["n1a"] == 0
            else:
                assert got["t1d_p1"] == 0.0 and got["n1a"] == 1.75
    # the literals themselves: the folded list is the unfolded one folded
    assert _t(*cases[((2, 2), False)][:2]) == pytest.approx(0.27942452264263223, rel=1e-14)
    assert _t(*cases[((3, 2), True)][:2]) == pytest.approx(0.6017401880563651, rel=1e-14)
    # T2D is pooled_t2d(residuals(X, b)) of the folded grids
    g = SP.project_np(p, recs, PU.Cfg(2, 2), 3, 2, [0, -1], [0, 1], 2)[0]
    res = SP.residuals(SP.fold_projected(g[0]), SP.fold_projected(g[1]))
    assert SP.pooled_t2d(res) == pytest.approx(_t(*cases[((3, 2), True)][:2]), rel=1e-13)


def test_anchor_full_size_against_the_oracle():
    """m = (36, 28) on fully called data: every weight is 1, the projected grids are the integer spectra, and the
    closed form is the scan's T2D / T1D wherever those are finite and non-zero (oracle.clr2d / clr1d)."""
    from oracle import sfs_oracle as O
    p = PU.genome(N1P, N2P, None, lengths=[255, 2049], full=True)
    recs = PS.records(p, 300)
    assert len(recs) == 6 and (recs["chrom"] == 1).all()
    worst = [0.0, 0.0, 0.0]
    for fold in (True, False):
        ocfg = O.Cfg(N1P, N2P, None, fold)
        tw = SP.project_scan_np(p, recs, PU.Cfg(N1P, N2P, fold=fold), 36, 28)
        chrom = np.arange(int(p.chrom_off[1]), int(p.chrom_off[2]))
        bg2 = O.sfs2d(p, chrom, ocfg)
        bg1 = [O.fold1d(O.sfs1d(p, chrom, w, ocfg)) for w in (1, 2)]
        for r, t in zip(recs, tw):
            idx = np.arange(int(r["begin"]), int(r["end"]))
            want = [O.clr2d(O.sfs2d(p, idx, ocfg), bg2)] + \
                   [O.clr1d(O.fold1d(O.sfs1d(p, idx, w, ocfg)), bg1[w - 1]) for w in (1, 2)]
            assert t["n_dropped"] == 0 and t["n_used"] == O.sfs2d(p, idx, ocfg).sum()
            for k, (f, w) in enumerate(zip(("t2d", "t1d_p1", "t1d_p2"), want)):
                assert w is not None and math.isfinite(w) and w != 0.0
                rel = abs(float(t[f]) - float(w)) / abs(float(w))
                worst[k] = max(worst[k], rel)
                assert rel <= 1e-10, (f, fold, float(t[f]), float(w))
    print("anchor: worst relative difference twin - oracle", worst)


def test_inf_nan_and_none_rules():
    p, recs = _tiny()
    cfg = PU.Cfg(2, 2, fold=False)
    # a background that lacks a touched bin: records against a "chromosome" of their own
    from sfs2d.pack import PackedSNPs
    q = PackedSNPs(p.counts, p.pos, np.array([0, 3, 6]), ["c1", "c2"], p.ann_id, p.ann_names)
    recs2 = recs.copy()
    recs2["chrom"] = [0, 1]
    own = SP.project_scan_np(q, recs2, cfg, 3, 2)
    assert abs(own["t2d"][0]) < 1e-15 and abs(own["t2d"][1]) < 1e-15          # a window that is its background
    cross = SP.project_scan_np(q, recs2, cfg, 3, 2, bg_chrom=1)
    assert cross["t2d"][0] == math.inf and abs(cross["t2d"][1]) < 1e-15         # S3's bin (3, 2) is not in S4 .. S6
    assert cross["t1d_p1"][0] != math.inf and not math.isnan(cross["t1d_p1"][0])
    # N = 0: every member dropped (m1 = 4 > n1 = 3), or no member at all; flagged records: the flags alone
    one = np.zeros(3, L.WINDOW_DTYPE)
    one["begin"], one["end"], one["flags"] = [1, 2, 0], [2, 2, 3], [0, 0, L.W_EMPTY]
    got = SP.project_scan_np(p, one, cfg, 4, 2)
    assert (got["n_used"][0], got["n_dropped"][0]) == (0, 1) and math.isnan(got["t2d"][0]) and got["n2"][0] == 0
    assert (got["n_used"][1], got["n_dropped"][1]) == (0, 0) and math.isnan(got["t2d"][1])
    assert got["flags"][2] == L.W_EMPTY and got["t2d"][2] == 0 and got["n_used"][2] == 0
    # B = 0: a background without a used SNP
    r = PackedSNPs(p.counts[[1, 0, 2]], p.pos[:3], np.array([0, 1, 3]), ["c1", "c2"], p.ann_id[:3], p.ann_names)
    two = np.zeros(1, L.WINDOW_DTYPE)
    two["begin"], two["end"], two["chrom"] = 1, 3, 1
    got = SP.project_scan_np(r, two, cfg, 4, 2, bg_chrom=0)
    assert got["n_used"][0] == 2 and got["n2"][0] > 0 and math.isnan(got["t2d"][0])
    with pytest.raises(ValueError):
        SP.project_scan_np(p, recs, cfg, 3, 2, bg_chrom=1)
    with pytest.raises(ValueError):
        SP.project_scan_np(p, recs, cfg, 5, 2)


def test_project_scan_rows():
    recs = np.zeros(6, L.WINDOW_DTYPE)
    recs["snp_count"] = [10, 11, 12, 13, 0, 15]
    st = np.zeros(6, L.PROJSTAT_DTYPE)
    st["t2d"] = [5.0, math.nan, math.inf, math.inf, 0.0, 3.0]
    st["t1d_p1"] = [1.0, 2.0, math.inf, 1.0, 0.0, math.nan]
    st["t1d_p2"] = [2.0, 3.0, 4.0, 2.0, 0.0, 1.5]
    st["n_used"], st["n_dropped"] = [9, 0, 8, 7, 0, 6], [1, 11, 4, 6, 0, 9]
    st["flags"][4] = L.W_EMPTY
    rows = SP.project_scan_rows(recs, st, ["a", "b", "c", None, "empty", "f"])
    assert list(rows) == ["a", "b", "c", "empty", "f"] and all(list(r) == SP.PROJSCAN_COLUMNS for r in rows.values())
    assert rows["a"] == {"snp_count": 10, "n_used": 9, "n_dropped": 1, "T2D_proj": 5.0, "T1D_pop1_proj": 1.0,
                         "T1D_pop2_proj": 2.0, "new_term_pop1_proj": 4.0, "new_term_pop2_proj": 3.0, "T2D_diff_proj": 3.5}
    b = rows["b"]
    assert b["T2D_proj"] is None and b["T1D_pop1_proj"] == 2.0 and b["new_term_pop1_proj"] is None and b["T2D_diff_proj"] is None
    c = rows["c"]      # +inf stays; inf - inf has no value
    assert c["T2D_proj"] == math.inf and c["new_term_pop1_proj"] is None and c["new_term_pop2_proj"] == math.inf
    assert c["T2D_diff_proj"] is None
    assert all(rows["empty"][k] is None for k in SP.PROJSCAN_COLUMNS[3:]) and rows["empty"]["snp_count"] == 0
    f = rows["f"]
    assert f["T1D_pop1_proj"] is None and f["new_term_pop1_proj"] is None and f["new_term_pop2_proj"] == 1.5
    assert f["T2D_diff_proj"] is None
    # the twin's records go through the same function
    p, r2 = _tiny()
    tw = SP.project_scan_np(p, r2, PU.Cfg(2, 2), 3, 2)
    rows = SP.project_scan_rows(r2, tw, ["w0", "w1"])
    assert rows["w0"]["T2D_proj"] == float(tw["t2d"][0]) and rows["w0"]["T1D_pop2_proj"] is None


# ------------------------------------------------------------------------------------------------- arguments

def test_cli_project_scan_argument_errors(capsys):
    from sfs2d import cli
    for argv, msg in ((["--project-scan", "24"], "--project-scan '24': expected M1,M2"),
                      (["--project-scan", "a,b"], "expected M1,M2"),
                      (["--project-scan", "1,20"], "2 <= M1 <= 36"),
                      (["--project-scan", "24,29"], "2 <= M2 <= 28"),
                      (["--project-scan", "12,12", "--pop1-size", "5"], "2 <= M1 <= 10"),
                      # --project alone stays the error it was
                      (["--project", "24,20"], "--project applies to --outlier-spectra / --region-spectra: give one of them"),
                      (["--project", "24,20", "--project-scan", "24,20"], "--project applies to --outlier-spectra"),
                      (["--project", "24", "--outlier-spectra", "T2D:0.9"], "--project '24': expected M1,M2")):
        with pytest.raises(SystemExit) as ei:
            cli.main(["no.vcf", "no.popmap"] + argv)
        assert ei.value.code == 2
        assert msg in capsys.readouterr().err, argv
    assert cli.parse_project("24,20", 18, 14, "--project-scan") == (24, 20)


def test_class_projected_scan_argument_errors():
    import twoDSFS_class as T
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=18, pop2_size=14)
    for bad in ((1, 20), (37, 20), (24, 29), (24,), "24,20", 24, None):
        with pytest.raises(ValueError):
            obj.projected_scan({}, bad, window_size=20000)
    dist = T.LikelihoodInference_jointSFS(None, None, distributed=True)
    with pytest.raises(NotImplementedError):
        dist.projected_scan({}, (24, 20), window_size=20000)
    p = PU.genome(N1P, N2P, None, lengths=[65])
    for kw in ({}, {"window_size": 20000, "snp_window_size": 100}, {"snp_window_size": 100, "step_size": 10}):
        with pytest.raises(ValueError):
            obj.projected_scan(p, (24, 20), **kw)
    with pytest.raises(ValueError, match="Background chromosome"):
        obj.projected_scan(p, (24, 20), window_size=20000, background_chromosome="nope")


def test_exports_and_header():
    names = ("sfs2d_plan_project_scan", "sfs2d_plan_project_scan_read")
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "sfs2d.h")).read()
    lib = L.lib()
    for name in names:
        assert name in L.EXPORTS and re.search(rf"^int {name}\(", hdr, re.M) and getattr(lib, name) is not None
    assert "#define SFS2D_ABI_VERSION 2" in hdr and "} sfs2d_projstat;" in hdr
    assert L.PROJSTAT_DTYPE.itemsize == 64
    assert L.PROJSTAT_DTYPE.names == ("t2d", "t1d_p1", "t1d_p2", "n2_fx", "n1a_fx", "n1b_fx", "n_used", "n_dropped",
                                      "flags", "e")
    body = hdr[hdr.index("typedef struct {\n  double t2d, t1d_p1, t1d_p2;\n  int64_t n2_fx"):hdr.index("} sfs2d_projstat;")]
    order = [body.index(f) for f in ("t2d", "n2_fx", "n1a_fx", "n1b_fx", "n_used", "n_dropped", "flags", " e;")]
    assert order == sorted(order)


# ------------------------------------------------------------------------------------------------- fixtures

def test_fixture_properties_of_the_gpu_genome():
    """On the twin's output, for the genome test_project_scan_gpu.py uses: an all-dropped window whose results are
    None; under a short background chromosome both +inf and finite windows; under per-chromosome backgrounds at
    least three quarters of the live windows with a finite non-zero T2D."""
    m = (7, 5)
    p = PS.genome(N1P, N2P, m)
    PU.assert_kinds(p, N1P, N2P, *m)
    cfg = PU.Cfg(N1P, N2P)
    recs = PS.records(p, 3)
    tw = PS.twin(p, recs, cfg, *m)
    at = int(p.chrom_off[-2]) + PS.ALL_DROPPED
    i = int(np.nonzero(recs["begin"] == at)[0][0])
    assert (tw["n_used"][i], tw["n_dropped"][i]) == (0, 3) and all(math.isnan(tw[f][i]) for f in ("t2d", "t1d_p1", "t1d_p2"))
    rows = SP.project_scan_rows(recs, tw, [f"w{k}" for k in range(len(recs))])
    assert all(rows[f"w{i}"][k] is None for k in SP.PROJSCAN_COLUMNS[3:]) and rows[f"w{i}"]["n_dropped"] == 3
    live = tw["n_used"] > 0
    ok = np.isfinite(tw["t2d"]) & (tw["t2d"] != 0)
    assert live.sum() > 4000 and 4 * int(ok[live].sum()) >= 3 * int(live.sum()), (int(ok[live].sum()), int(live.sum()))
    # the larger windows of the plan-kind tests, at the projection they use
    M = (24, 20)
    q = PS.genome(N1P, N2P, M)
    recs = PS.records(q, 65)
    per = PS.twin(q, recs, cfg, *M)
    ok = np.isfinite(per["t2d"]) & (per["t2d"] != 0)
    assert len(recs) > 200 and 4 * int(ok.sum()) >= 3 * len(recs)
    short = PS.twin(q, recs, cfg, *M, bg_chrom=4)      # 255 SNPs: its own three windows are finite
    assert int(q.chrom_off[5] - q.chrom_off[4]) == 255
    assert np.isinf(short["t2d"]).any() and np.isfinite(short["t2d"]).any() and not np.isnan(short["t2d"]).any()
