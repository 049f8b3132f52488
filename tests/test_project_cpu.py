"""The host side of the projected spectra (sfs2d_project_weights, sfs2d.spectra's projection helpers, the CLI's
--project): no GPU.  DESIGN.md section 18."""
import csv
import ctypes as C
import math
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

import project_util as PU
from sfs2d import _lib as L
from sfs2d import spectra as SP


def _packed(rows, chrom_off=None, names=("c0",)):
    from sfs2d.pack import PackedSNPs, pack_counts
    a = np.array(rows, np.int64)
    n = len(a)
    return PackedSNPs(pack_counts(a[:, 0], a[:, 1], a[:, 2], a[:, 3]), np.arange(1, n + 1, dtype=np.uint32),
                      np.array([0, n] if chrom_off is None else chrom_off, np.int64), list(names),
                      np.zeros(n, np.uint16), ["a0", "a1"])


# ------------------------------------------------------------------------------------------------- weights

def test_weights_against_exact_rationals():
    """Every (n, a, m) with n <= 72 and a seeded sample of 20,000 with n up to 510: rows sum to 1, weights outside
    the support are exactly 0, m = n is exactly the indicator of j = a; the worst relative error over weights above
    1e-30 is printed (R = 4 x that is the GPU tests' relative tolerance)."""
    count = [0]

    def check(n, a, m, got, want):
        count[0] += 1
        lo, hi = max(0, m - (n - a)), min(m, a)
        assert not got[:lo].any() and not got[hi + 1:].any(), (n, a, m)            # exactly 0 outside the support
        assert (got[lo:hi + 1] > 0).all() or want[lo:hi + 1].min() < 1e-300, (n, a, m)
        assert abs(math.fsum(got.tolist()) - 1.0) <= 1e-11, (n, a, m)
        if m == n:
            assert got[a] == 1.0 and got.sum() == 1.0, (n, a, m)
        if lo == hi:
            assert got[lo] == 1.0, (n, a, m)
    worst = PU.weights_error(PU.weight_cases(), check)
    print(f"\nsfs2d_project_weights: worst relative error {worst:.3e} over {count[0]} cases; R = {4 * worst:.3e}")
    assert count[0] == sum((n + 1) ** 2 for n in range(73)) + 20000
    # (the ln k! / exp formula in doubles: an error of a few ulp of ln 510! ~ 2,670, i.e. ~1e-12; a formula gone
    # wrong is off by far more)
    assert 0.0 < worst < 1e-10


def test_weights_literals_and_refusals():
    lib = L.lib()
    w = np.full(8, 7.0)
    assert lib.sfs2d_project_weights(5, 2, 3, L.ptr(w)) == 0
    assert np.allclose(w[:4], [0.1, 0.6, 0.3, 0.0], rtol=1e-13, atol=0) and w[3] == 0.0 and (w[4:] == 7.0).all()
    assert [F(x) for x in SP.project_weights_exact(5, 2, 3)] == [F(1, 10), F(3, 5), F(3, 10), F(0)]
    assert lib.sfs2d_project_weights(0, 0, 0, L.ptr(w)) == 0 and w[0] == 1.0
    assert lib.sfs2d_project_weights(510, 255, 510, L.ptr(np.zeros(511))) == 0
    for n, a, m in ((5, 6, 3), (5, 2, 6), (511, 2, 3), (-1, 0, 0), (5, -1, 3), (5, 2, -1)):
        assert lib.sfs2d_project_weights(n, a, m, L.ptr(w)) == L.E_ARG, (n, a, m)
    assert lib.sfs2d_project_weights(5, 2, 3, None) == L.E_ARG
    with pytest.raises(ValueError):
        SP.project_weights_exact(5, 6, 3)


# ------------------------------------------------------------------------------------------------- the twin

SNPS = [(3, 1, 4, 0),    # 0: fully called (4, 4), alt (1, 0)
        (2, 1, 2, 2),    # 1: one allele missing in population 1: n1 = 3
        (4, 0, 4, 0),    # 2: (0, 0): not a member
        (0, 4, 0, 4),    # 3: folded to (0, 0): not a member of a folding plan; unfolded a member, alt (4, 4)
        (1, 0, 2, 2)]    # 4: n1 = 1: a member, dropped by every projection


def test_project_np_literals():
    """A 2 / 2 sample projected to (2, 2) and to (3, 2), with one missing allele."""
    p = _packed(SNPS)
    recs = np.zeros(3, L.WINDOW_DTYPE)
    recs["begin"], recs["end"] = [0, 0, 1], [5, 99, 2]        # (the second range is clamped to the data set)
    recs["flags"][1] = L.W_EMPTY
    g, u, d = SP.project_np(p, recs, PU.Cfg(2, 2), 2, 2, exact=True)
    assert g.shape == (3, 3, 3) and u.tolist() == [2, 0, 1] and d.tolist() == [1, 0, 0]
    # SNP 0: h(.; 4, 1, 2) = (1/2, 1/2, 0) x h(.; 4, 0, 2) = (1, 0, 0)
    # SNP 1: h(.; 3, 1, 2) = (1/3, 2/3, 0) x h(.; 4, 2, 2) = (1/6, 2/3, 1/6)
    s1 = [[F(1, 18), F(2, 9), F(1, 18)], [F(1, 9), F(4, 9), F(1, 9)], [0, 0, 0]]
    assert g[2].tolist() == s1
    assert g[0].tolist() == [[F(1, 2) + F(1, 18), F(2, 9), F(1, 18)], [F(1, 2) + F(1, 9), F(4, 9), F(1, 9)], [0, 0, 0]]
    assert not g[1].any()
    # (3, 2): SNP 1 has n1 = m1 = 3, the indicator of a1 = 1; SNP 0: h(.; 4, 1, 3) = (1/4, 3/4, 0, 0)
    g, u, d = SP.project_np(p, recs, PU.Cfg(2, 2), 3, 2, exact=True)
    assert g.shape == (3, 4, 3) and u.tolist() == [2, 0, 1] and d.tolist() == [1, 0, 0]
    assert g[2].tolist() == [[0, 0, 0], [F(1, 6), F(2, 3), F(1, 6)], [0, 0, 0], [0, 0, 0]]
    assert g[0].tolist() == [[F(1, 4), 0, 0], [F(3, 4) + F(1, 6), F(2, 3), F(1, 6)], [0, 0, 0], [0, 0, 0]]
    # (4, 4): the SNP with the missing allele is dropped too
    g, u, d = SP.project_np(p, recs, PU.Cfg(2, 2), 4, 4, exact=True)
    assert u.tolist() == [1, 0, 0] and d.tolist() == [2, 0, 1] and g[0][1, 0] == 1 and g[0].sum() == 1
    # without the fold SNP 3 is a member: the raw alt counts are projected, (4, 4) -> bin (2, 2)
    gn, un, dn = SP.project_np(p, recs, PU.Cfg(2, 2, fold=False), 2, 2, exact=True)
    assert un.tolist() == [3, 0, 1] and gn[0][2, 2] == 1 and gn[0].sum() == 3
    # floats: one conversion per bin; groups: a record twice counts twice, a chromosome entry, an empty group
    f, u, d = SP.project_np(p, recs, PU.Cfg(2, 2), 2, 2, [2, 2, -1, 1], [0, 0, 2, 0], 4)
    assert f.dtype == np.float64 and f[0].tolist() == [[float(2 * x) for x in row] for row in s1]
    assert u.tolist() == [2, 0, 2, 0] and d.tolist() == [0, 0, 1, 0] and not f[1].any() and not f[3].any()
    assert np.array_equal(f[2], SP.project_np(p, recs, PU.Cfg(2, 2), 2, 2)[0][0])
    for bad in ((1, 2), (2, 5), (5, 2)):
        with pytest.raises(ValueError):
            SP.project_np(p, recs, PU.Cfg(2, 2), *bad)
    with pytest.raises(ValueError):
        SP.project_np(p, recs, PU.Cfg(2, 2), 2, 2, [-2], [0], 1)       # one chromosome only
    with pytest.raises(ValueError):
        SP.project_np(p, recs, PU.Cfg(2, 2), 2, 2, [3], [0], 1)


FIXTURES = [(18, 14, (2, 2), None, False), (18, 14, (7, 5), None, False), (18, 14, (24, 20), None, False),
            (18, 14, (36, 28), None, True), (100, 75, (160, 120), [2049, 1000, 257], False),
            (127, 127, (254, 254), [2049, 1000, 257], True)]


@pytest.mark.parametrize("n1p,n2p,m,lengths,full", FIXTURES, ids=[f"{f[2][0]}x{f[2][1]}" for f in FIXTURES])
def test_gpu_fixtures_hold_every_kind(n1p, n2p, m, lengths, full):
    """The genomes of test_project_gpu.py, on the twin's output: every planted kind is there and does what it is
    planted for, and no whole chromosome of 255 SNPs or more loses more than 25 % of its members -- a condition
    of the fixtures, not a measurement (the full sizes run on the fully called copy)."""
    p = PU.genome(n1p, n2p, m, lengths=lengths, full=full)
    PU.assert_kinds(p, n1p, n2p, *m, missing=not full)
    PU.assert_dropped_share(p, PU.Cfg(n1p, n2p), *m)
    PU.assert_dropped_share(p, PU.Cfg(n1p, n2p, fold=False), *m)


# ------------------------------------------------------------------------------------------------- host helpers

def test_fold_projected_with_tie():
    g = np.arange(15, dtype=np.int64).reshape(3, 5)            # m = (2, 4): folded where 2 (i + j) > 6
    f = SP.fold_projected(g)
    assert f.dtype == np.int64
    assert f.tolist() == [[0 + 14, 1 + 13, 2 + 12, 3, 0], [5 + 9, 6 + 8, 7, 0, 0], [10 + 4, 11, 0, 0, 0]]      # the ties 3, 7, 11 stay
    assert f.sum() == g.sum()
    h = np.arange(12, dtype=np.float64).reshape(3, 4)          # m = (2, 3), odd sum: no tie
    assert SP.fold_projected(h).tolist() == [[11.0, 11.0, 11.0, 0.0], [11.0, 11.0, 0.0, 0.0], [11.0, 0.0, 0.0, 0.0]]
    both = SP.fold_projected(np.stack([g, 2 * g]))
    assert np.array_equal(both[0], f) and np.array_equal(both[1], 2 * f)
    ex = np.array([[F(1, 3), F(1, 6)], [F(1, 4), F(1, 4)]], object)
    assert SP.fold_projected(ex).tolist() == [[F(1, 3) + F(1, 4), F(1, 6)], [F(1, 4), 0]]
    assert SP.fold1d_projected(np.arange(5)).tolist() == [4, 4, 2, 0, 0]
    assert SP.fold1d_projected(np.arange(4.0)).tolist() == [3.0, 3.0, 0.0, 0.0]


def test_marginals_are_1d_projections():
    """The marginals of the joint projection are the 1D projections of the used SNPs, exactly."""
    p = PU.genome(18, 14, (7, 5), lengths=[257])
    g, u, d = SP.project_np(p, None or np.zeros(0, L.WINDOW_DTYPE), PU.Cfg(18, 14), 7, 5, [-1], [0], 1, exact=True)
    s1, s2 = SP.projected_marginals(g[0])
    r1, a1, r2, a2 = SP._members(p, 0, p.n, PU.Cfg(18, 14), 18, 14, True)
    use = (r1 + a1 >= 7) & (r2 + a2 >= 5)
    assert int(use.sum()) == int(u[0]) > 150 and int((~use).sum()) == int(d[0]) > 0
    for s, r, a, m in ((s1, r1, a1, 7), (s2, r2, a2, 5)):
        want = [F(0)] * (m + 1)
        for q, b in zip(r[use].tolist(), a[use].tolist()):
            want = [x + y for x, y in zip(want, SP.project_weights_exact(q + b, b, m))]
        assert s.tolist() == want and sum(want) == int(u[0])
    f1 = SP.fold1d_projected(s1)
    assert f1[:4].tolist() == [s1[j] + s1[7 - j] for j in range(4)] and not f1[4:].any()


def test_float_grids_through_residuals_and_files(tmp_path):
    fg = np.array([[0.5, 2.25, 0.0], [1.0, 0.0, 3.125], [0.0, 4.0, 0.75]])      # inner: N = 10.375
    bg = np.array([[5.5, 10.0, 5.0], [2.5, 5.0, 10.0], [5.0, 20.25, 1.0]])      # inner: B = 57.75
    r = SP.residuals(fg, bg)
    assert r["fg_count"].dtype == np.float64 and np.array_equal(r["fg_count"], fg) and np.array_equal(r["bg_count"], bg)
    assert r["fg_p"][0, 1] == 2.25 / 10.375 and r["bg_p"][2, 1] == 20.25 / 57.75
    want = 2 * sum(x * (math.log(x / 10.375) - math.log(b / 57.75))
                   for x, b in zip(fg.ravel()[1:-1].tolist(), bg.ravel()[1:-1].tolist()) if x)
    assert SP.pooled_t2d(r) == pytest.approx(want, rel=1e-13)
    rows = SP.residual_rows(r)
    assert len(rows) == 9 and rows[0][:4] == [0, 0, 0.5, 5.5] and rows[1][:4] == [0, 1, 2.25, 10.0]
    assert all(isinstance(row[2], float) and isinstance(row[3], float) for row in rows)      # nothing truncated
    path = tmp_path / "r.csv"
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(SP.RESIDUAL_COLUMNS)
        w.writerows(rows)
    with open(path, newline="") as fh:
        back = list(csv.DictReader(fh))
    assert [float(b["fg_count"]) for b in back] == fg.ravel().tolist()
    assert [float(b["bg_count"]) for b in back] == bg.ravel().tolist()
    # .fs: doubles survive exactly, thirds included
    g = np.array([[1 / 3, 2.0], [0.1, 1e-17], [5.5, 0.0]])
    SP.write_dadi_fs(tmp_path / "p.fs", g, True, ("uv", "bv"))
    back, folded, ids, mask = SP.read_dadi_fs(tmp_path / "p.fs")
    assert back.dtype == np.float64 and np.array_equal(back, g) and folded and back.shape == (3, 2)
    assert mask.tolist() == [[1, 0], [0, 1], [1, 1]]      # (0, 0), the last bin, and i + j > (2 + 1) // 2


def test_integer_path_is_byte_identical(tmp_path):
    """The integer grids' residual table and .fs files, byte for byte as before float grids were carried (the
    expected text is a copy made before the change)."""
    fg = np.array([[9, 2, 0], [1, 0, 3], [0, 4, 7]], np.int64)
    bg = np.array([[5, 10, 5], [5, 5, 10], [5, 20, 1]], np.int64)
    res = SP.residuals(fg, bg)
    rows = SP.residual_rows(res)
    assert [type(v) for v in rows[0]] == [int, int, int, int, float, float, float, float]
    with open(tmp_path / "r.csv", "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(SP.RESIDUAL_COLUMNS)
        w.writerows(rows)
    assert (tmp_path / "r.csv").read_bytes() == (
        b"x1,x2,fg_count,bg_count,fg_p,bg_p,diff,t2d_term\r\n"
        b"0,0,9,5,0.9,0.08333333333333333,0.8166666666666667,0.0\r\n"
        b"0,1,2,10,0.2,0.16666666666666666,0.033333333333333354,0.7292862271758187\r\n"
        b"0,2,0,5,0.0,0.08333333333333333,-0.08333333333333333,0.0\r\n"
        b"1,0,1,5,0.1,0.08333333333333333,0.016666666666666677,0.3646431135879098\r\n"
        b"1,1,0,5,0.0,0.08333333333333333,-0.08333333333333333,0.0\r\n"
        b"1,2,3,10,0.3,0.16666666666666666,0.13333333333333333,3.526719989412713\r\n"
        b"2,0,0,5,0.0,0.08333333333333333,-0.08333333333333333,0.0\r\n"
        b"2,1,4,20,0.4,0.3333333333333333,0.06666666666666671,1.4585724543516383\r\n"
        b"2,2,7,1,0.7,0.016666666666666666,0.6833333333333332,0.0\r\n")
    SP.write_dadi_fs(tmp_path / "a.fs", fg, True, ("uv", "bv"))
    assert (tmp_path / "a.fs").read_bytes() == b'3 3 folded "uv" "bv"\n9 2 0 1 0 3 0 4 7\n1 0 0 0 0 1 0 1 1\n'


# ------------------------------------------------------------------------------------------------- arguments

def test_cli_project_argument_errors(capsys):
    from sfs2d import cli
    for argv, msg in ((["--project", "24,20"], "--outlier-spectra / --region-spectra"),
                      (["--project", "24", "--outlier-spectra", "T2D:0.9"], "M1,M2"),
                      (["--project", "a,b", "--outlier-spectra", "T2D:0.9"], "M1,M2"),
                      (["--project", "1,20", "--outlier-spectra", "T2D:0.9"], "2 <= M1 <= 36"),
                      (["--project", "24,29", "--outlier-spectra", "T2D:0.9"], "2 <= M2 <= 28"),
                      (["--project", "37,20", "--regions", "x.bed", "--region-spectra"], "2 <= M1 <= 36"),
                      (["--project", "12,12", "--pop1-size", "5", "--outlier-spectra", "T2D:0.9"], "2 <= M1 <= 10")):
        with pytest.raises(SystemExit) as ei:
            cli.main(["no.vcf", "no.popmap"] + argv)
        assert ei.value.code == 2
        assert msg in capsys.readouterr().err
    assert cli.parse_project("24,20", 18, 14) == (24, 20) and cli.parse_project(" 36 , 28 ", 18, 14) == (36, 28)
    assert cli._dropped_share(75, 25) == "25 of 100 SNPs dropped (25.00 %)" and cli._dropped_share(0, 0) == "no SNPs"


def test_class_project_argument_errors():
    import twoDSFS_class as T
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=18, pop2_size=14)
    for bad in ((1, 20), (37, 20), (24, 29), (24,), "24,20", 24):
        with pytest.raises(ValueError):
            obj.window_spectra({}, window_size=20000, project=bad)
        with pytest.raises(ValueError):
            obj.outlier_spectra({}, window_size=20000, project=bad)
    dist = T.LikelihoodInference_jointSFS(None, None, distributed=True)
    with pytest.raises(NotImplementedError):
        dist.window_spectra({}, window_size=20000, project=(24, 20))
    with pytest.raises(NotImplementedError):
        dist.outlier_spectra({}, window_size=20000, project=(24, 20))


def test_exports_and_header():
    for name in ("sfs2d_plan_project", "sfs2d_plan_project_read", "sfs2d_project_weights"):
        assert name in L.EXPORTS
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "sfs2d.h")).read()
    for name in ("sfs2d_plan_project", "sfs2d_plan_project_read", "sfs2d_project_weights"):
        assert re.search(rf"^int {name}\(", hdr, re.M), name
    assert "#define SFS2D_ABI_VERSION 2" in hdr and "#define SFS2D_PROJ_ROW_WORDS(m1, m2)" in hdr
    assert L.proj_row_words(2, 2) == 11 and L.proj_row_words(254, 254) == 255 * 255 + 2
    assert L.proj_row_words(160, 120) * 8 == 155864        # the largest row the tests put into LDS
    lib = L.lib()
    for name in ("sfs2d_plan_project", "sfs2d_plan_project_read", "sfs2d_project_weights"):
        assert getattr(lib, name) is not None
