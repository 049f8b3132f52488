"""The host side of the window spectra (sfs2d.spectra, the CLI's new arguments): no GPU."""
import math

import numpy as np
import pytest

from sfs2d import _lib as L
from sfs2d import spectra as SP


def _packed(rows, chrom_off=None, pos=None, ann=None):
    from sfs2d.pack import PackedSNPs, pack_counts
    a = np.array(rows, np.int64)
    n = len(a)
    return PackedSNPs(pack_counts(a[:, 0], a[:, 1], a[:, 2], a[:, 3]),
                      np.arange(1, n + 1, dtype=np.uint32) if pos is None else np.asarray(pos, np.uint32),
                      np.array([0, n] if chrom_off is None else chrom_off, np.int64), ["c0"],
                      np.zeros(n, np.uint16) if ann is None else np.asarray(ann, np.uint16), ["a0", "a1"])


class _Cfg:
    def __init__(self, n1p, n2p, fold=True, ann_want=-1, start_position=None, end_position=None):
        self.n1p, self.n2p, self.fold, self.ann_want = n1p, n2p, fold, ann_want
        self.start_position, self.end_position = start_position, end_position


def test_row_words_and_split_row():
    assert L.spec_row_words(2, 1) == 5 * 3 + 2 + 1 + 2 == 20
    assert L.spec_row_words(25, 25) == 51 * 51 + 52
    row = np.arange(20, dtype=np.int64)
    g, f1, f2 = SP.split_row(row, 2, 1)
    assert g.shape == (5, 3) and g[0].tolist() == [0, 1, 2] and g[4, 2] == 14
    assert f1.tolist() == [15, 16, 17] and f2.tolist() == [18, 19]
    with pytest.raises(ValueError):
        SP.split_row(row[:-1], 2, 1)


def test_window_spectra_np_literals():
    """pop (2, 2): n1 = n2 = 4, grid 5 x 5, the fold when alt1 + alt2 > 4; inner 1D bin 1 alone."""
    snps = [(3, 1, 4, 0),    # 0: key (1, 0); pop-1 folded bin 1
            (0, 4, 0, 4),    # 1: folded to (0, 0): skipped; unfolded the last bin (4, 4); 1D bins 0: not exported
            (1, 3, 2, 2),    # 2: alt sum 5 > 4: folded to the refs (1, 2); 1D pop-1 min(3, 1) = 1, pop-2 bin 2 = n_p
            (2, 2, 2, 2),    # 3: alt sum 4: a tie, not folded: (2, 2); 1D bins 2 = n_p: not exported
            (4, 0, 4, 0),    # 4: (0, 0): skipped
            (4, 2, 4, 1),    # 5: over-called (6 and 5 alleles), alt sum 3: key (2, 1); 1D pop-1 bin 2, pop-2 bin 1
            (4, 3, 4, 2)]    # 6: over-called, alt sum 5 > 4: folded to the refs (4, 4), the last bin; 1D 1 and 2
    p = _packed(snps)
    recs = np.zeros(4, L.WINDOW_DTYPE)
    recs["begin"], recs["end"] = [0, 3, 0, 5], [3, 7, 7, 99]      # (the last range is clamped to the data set)
    recs["flags"][2] = L.W_EMPTY
    grid = lambda *keys: [int(k in keys) for k in range(25)]
    fold = SP.window_spectra_np(p, recs, _Cfg(2, 2))
    assert fold.shape == (4, 31)
    assert fold[0].tolist() == grid(5, 7) + [0, 2, 0] + [0, 0, 0]
    assert fold[1].tolist() == grid(12, 11, 24) + [0, 1, 0] + [0, 1, 0]
    assert not fold[2].any()
    assert fold[3].tolist() == grid(11, 24) + [0, 1, 0] + [0, 1, 0]
    nofold = SP.window_spectra_np(p, recs, _Cfg(2, 2, fold=False))
    assert nofold[0].tolist() == grid(5, 24, 17) + [0, 2, 0] + [0, 0, 0]
    assert nofold[1].tolist() == grid(12, 11, 17) + [0, 1, 0] + [0, 1, 0]
    # groups: a record listed twice is counted twice, an empty record adds nothing, an empty group is zero
    pooled = SP.window_spectra_np(p, recs, _Cfg(2, 2), [1, 0, 1, 2], [0, 2, 0, 2], 4)
    assert np.array_equal(pooled[0], 2 * fold[1]) and np.array_equal(pooled[2], fold[0])
    assert not pooled[1].any() and not pooled[3].any()
    assert SP.window_spectra_np(p, recs, _Cfg(2, 2), [], [], 2).shape == (2, 31)
    # the filters take SNPs out: positions 1 .. 7, annotation 1 on SNPs 0, 2, 5
    q = _packed(snps, ann=[1, 0, 1, 0, 0, 1, 0])
    f = SP.window_spectra_np(q, recs[:1], _Cfg(2, 2, ann_want=1, start_position=2))
    assert f[0].tolist() == grid(7) + [0, 1, 0] + [0, 0, 0]
    with pytest.raises(ValueError):
        SP.window_spectra_np(p, recs, _Cfg(2, 2), [4], [0], 1)
    with pytest.raises(KeyError):      # an alt count above 2 pop_size: the reference's KeyError
        SP.window_spectra_np(_packed([(0, 1, 0, 5)]), recs[:1], _Cfg(2, 2))      # (folded to (0, 0): the 2D grid skips it)


def test_select_top():
    rows = {f"w{i}": {"T2D": v} for i, v in enumerate([1.0, None, 5.0, float("nan"), 3.0, 5.0, float("inf"), 2.0, 0.0, 4.0])}
    # candidates 1, 5, 3, 5, inf, 2, 0, 4 (8 of them); q = 0.5 -> quantile "higher" = 4
    assert SP.select_top(rows, "T2D", 0.5) == ["w2", "w5", "w6", "w9"]
    # ties at the threshold are all in, in scan order; None and NaN never are; inf is the most extreme
    assert SP.select_top(rows, "T2D", 0.7) == ["w2", "w5", "w6"]
    assert SP.select_top(rows, "T2D", 0.99) == ["w6"]
    assert SP.select_top(rows, "T2D", 0.01) == ["w0", "w2", "w4", "w5", "w6", "w7", "w9"]
    vals = np.array([1.0, 5.0, 3.0, 5.0, np.inf, 2.0, 0.0, 4.0])
    for q in (0.1, 0.25, 0.5, 0.8, 0.9):
        thr = np.quantile(vals, q, method="higher")
        assert len(SP.select_top(rows, "T2D", q)) == int((vals >= thr).sum())
    for q in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            SP.select_top(rows, "T2D", q)
    with pytest.raises(ValueError):
        SP.select_top({"a": {"T2D": None}, "b": {"T2D": float("nan")}}, "T2D", 0.5)
    with pytest.raises(ValueError):
        SP.select_top(rows, "FST", 0.5)      # no row has the key


def test_residuals_literal():
    fg = np.array([[9, 2, 0], [1, 0, 3], [0, 4, 7]], np.int64)      # inner: 2 0 1 0 3 0 4 -> N = 10
    bg = np.array([[5, 10, 5], [0, 5, 10], [5, 20, 1]], np.int64)   # inner: 10 5 0 5 10 5 20 -> B = 55
    r = SP.residuals(fg, bg)
    assert np.array_equal(r["fg_count"], fg) and np.array_equal(r["bg_count"], bg)
    assert r["fg_p"].tolist() == [[0.9, 0.2, 0.0], [0.1, 0.0, 0.3], [0.0, 0.4, 0.7]]
    assert r["bg_p"][0, 1] == 10 / 55 and r["bg_p"][2, 2] == 1 / 55
    assert np.array_equal(r["diff"], r["fg_p"] - r["bg_p"])
    t = r["t2d_term"]
    assert t[0, 0] == 0.0 and t[2, 2] == 0.0                         # the two bins the statistic does not read
    assert t[0, 2] == 0.0 and t[1, 1] == 0.0 and t[2, 0] == 0.0      # x = 0
    assert t[1, 0] == math.inf                                       # x > 0 where b = 0
    assert t[0, 1] == pytest.approx(2 * 2 * (math.log(0.2) - math.log(10 / 55)), rel=1e-14)
    assert t[2, 1] == pytest.approx(2 * 4 * (math.log(0.4) - math.log(20 / 55)), rel=1e-14)
    assert SP.pooled_t2d(r) == math.inf
    # without the b = 0 bin: the terms sum to the multinomial log-likelihood ratio
    bg[1, 0] = 5
    r = SP.residuals(fg, bg)
    x, b = fg.ravel()[1:-1], bg.ravel()[1:-1]
    want = 2 * sum(xi * (math.log(xi / 10) - math.log(bi / 60)) for xi, bi in zip(x.tolist(), b.tolist()) if xi)
    assert SP.pooled_t2d(r) == pytest.approx(want, rel=1e-13)
    rows = SP.residual_rows(r)
    assert [row[:4] for row in rows][:3] == [[0, 0, 9, 5], [0, 1, 2, 10], [0, 2, 0, 5]] and len(rows) == 9
    assert len(rows[0]) == len(SP.RESIDUAL_COLUMNS)
    # an empty foreground or background
    assert SP.pooled_t2d(SP.residuals(np.zeros((3, 3), np.int64), bg)) is None
    assert SP.pooled_t2d(SP.residuals(fg, np.zeros((3, 3), np.int64))) is None
    with pytest.raises(ValueError):
        SP.residuals(fg, bg[:2])


def test_dadi_fs_round_trip_and_mask(tmp_path):
    rng = np.random.default_rng(3)
    g = rng.integers(0, 50, (5, 7)).astype(np.int64)      # pop sizes (2, 3): n1p + n2p = 5
    path = tmp_path / "a.fs"
    SP.write_dadi_fs(path, g, True, ("uv", "bv"))
    lines = path.read_text().splitlines()
    assert len(lines) == 3 and lines[0] == '5 7 folded "uv" "bv"'
    assert lines[1].split() == [str(v) for v in g.ravel()]
    back, folded, ids, mask = SP.read_dadi_fs(path)
    assert back.dtype == np.int64 and np.array_equal(back, g) and folded and ids == ("uv", "bv")
    want = np.zeros((5, 7), np.int64)
    for i in range(5):
        for j in range(7):
            want[i, j] = int((i, j) in ((0, 0), (4, 6)) or i + j > 5)
    assert np.array_equal(mask, want) and mask[2, 3] == 0 and mask[2, 4] == 1
    SP.write_dadi_fs(path, g, False, ("pop one", "p2"))
    back, folded, ids, mask = SP.read_dadi_fs(path)
    assert not folded and ids == ("pop one", "p2") and np.array_equal(back, g)
    assert mask.sum() == 2 and mask[0, 0] == mask[4, 6] == 1
    # proportions survive the trip exactly (repr of a double)
    f = g / g.sum()
    SP.write_dadi_fs(path, f, True)
    back = SP.read_dadi_fs(path)[0]
    assert back.dtype == np.float64 and np.array_equal(back, f)
    # comment lines ahead of the header, no mask line
    path.write_text('# made elsewhere\n2 2 unfolded "a" "b"\n0 1 2 0\n')
    back, folded, ids, mask = SP.read_dadi_fs(path)
    assert back.tolist() == [[0, 1], [2, 0]] and mask is None and ids == ("a", "b")
    path.write_text('2 2 unfolded\n0 1 2\n')
    with pytest.raises(ValueError):
        SP.read_dadi_fs(path)
    with pytest.raises(ValueError):
        SP.write_dadi_fs(path, g, True, ('a"b', "c"))


def test_cli_argument_errors(capsys):
    from sfs2d import cli
    for argv, msg in ((["--outlier-spectra", "T2D"], "KEY:Q"), (["--outlier-spectra", "T2D:high"], "(0, 1)"),
                      (["--outlier-spectra", "T2D:1.0"], "(0, 1)"), (["--outlier-spectra", "pi_pop1:0.9"], "KEY:Q"),
                      (["--outlier-spectra", "FST:0.99"], "--fst"), (["--region-spectra"], "--regions")):
        with pytest.raises(SystemExit) as ei:
            cli.main(["no.vcf", "no.popmap"] + argv)
        assert ei.value.code == 2
        assert msg in capsys.readouterr().err
    assert cli.parse_outlier_spec("T1D_p2:0.995") == ("T1D_p2", 0.995)
    assert cli._fmt_pct(0.99) == "1" and cli._fmt_pct(0.995) == "0.5" and cli._fmt_pct(0.8) == "20"


def test_exports_and_header():
    import os
    import re
    assert "sfs2d_plan_spectra" in L.EXPORTS and "sfs2d_plan_spectra_read" in L.EXPORTS
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "sfs2d.h")).read()
    assert re.search(r"^int sfs2d_plan_spectra\(", hdr, re.M) and re.search(r"^int sfs2d_plan_spectra_read\(", hdr, re.M)
    assert "#define SFS2D_ABI_VERSION 2" in hdr and "SFS2D_SPEC_ROW_WORDS" in hdr


def test_class_refuses_distributed():
    import twoDSFS_class as T
    obj = T.LikelihoodInference_jointSFS(None, None, distributed=True)
    with pytest.raises(NotImplementedError):
        obj.window_spectra({}, window_size=20000)
    with pytest.raises(NotImplementedError):
        obj.outlier_spectra({}, window_size=20000)
