"""Window spectra on the device (kernel k_spec_win, sfs2d_plan_spectra) against the oracle:
every comparison of spectra is exact integer equality with oracle.sfs2d / sfs1d / fold1d over the record's own
range under the plan's configuration (tests/spectra_util.py).

The genome has ~14,000 SNPs in chromosomes of 1, 63, 64, 65, 255, 256, 257, 2,047, 2,049 and 9,000 SNPs, pop
(12, 12) and (25, 25): a regions plan of whole chromosomes puts record ranges on, one below and one above a row of 64
SNPs, a workgroup row of 256 and the eight rows in flight (2,048).  The fixture's awkward SNPs -- (0, 0), last bin,
folded, fold tie, over-called, folded 1D bins 0 and n_p -- are asserted on the oracle in spectra_util.assert_kinds.
The larger grids (101 x 101, 201 x 151, 255 x 255) run at ~3,300 SNPs."""
import csv
import ctypes as C
import math
import os

import numpy as np
import pytest

import spectra_util as SU
from golden_util import GOLD, close
from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import post
from sfs2d import spectra as SP

pytestmark = pytest.mark.gpu

POPS = [(12, 12), (25, 25)]
BIG = [2049, 1000, 257]
FILT = {"start_position": 3000, "end_position": 400000, "ann_want": 1}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE", "SFS2D_SLOTS_ONCE"):
        monkeypatch.delenv(k, raising=False)


def _cfg(n1p=12, n2p=12, **kw):
    from sfs2d.engine import ScanConfig
    return ScanConfig(n1p=n1p, n2p=n2p, **kw)


def _whole_chroms(p):
    from sfs2d.regions import Regions
    return Regions(p.chrom_names, [(c, 0, (1 << 32) - 1, f"whole_{c}") for c in p.chrom_names])


def _check_each(p, pl, cfg, what=""):
    """Per-window export (rec = NULL, group i = record i) against the oracle; returns (records, rows)."""
    recs = pl.read()
    rows = pl.spectra()
    assert rows.shape == (max(1, pl.nrec), L.spec_row_words(cfg.n1p, cfg.n2p))
    SU.assert_rows(rows[:len(recs)], SU.expected(p, recs, SU.ocfg_of(cfg, p)), what)
    return recs, rows


def _check_invariants(p, recs, rows, cfg, bg_of_chrom, what=""):
    """What the records say about their windows' spectra: the four totals, and T2D / T1D recomputed by the oracle
    from the exported spectra against the chromosome's background."""
    nt = 0
    for r, row in zip(recs, rows):
        if int(r["flags"]) & (L.W_EMPTY | L.W_EXTRA):
            assert not row.any()
            continue
        g, f1, f2 = SP.split_row(row, cfg.n1p, cfg.n2p)
        assert int(r["n2_all"]) == int(g.sum()), (what, int(r["wid"]))
        assert int(r["n2"]) == int(g.ravel()[1:-1].sum()), (what, int(r["wid"]))
        assert int(r["n1a"]) == int(f1.sum()) and int(r["n1b"]) == int(f2.sum()), (what, int(r["wid"]))
        assert f1[0] == f1[-1] == f2[0] == f2[-1] == 0 and g[0, 0] == 0
        b2, b1a, b1b = bg_of_chrom(int(r["chrom"]))
        for which, want in ((2, O.clr2d(g, b2)), (1, O.clr1d(f1, b1a)), (0, O.clr1d(f2, b1b))):
            got = post._v(r, which)
            want = None if want is None else float(want)
            assert close(got, want), (what, int(r["chrom"]), int(r["wid"]), which, got, want)
            nt += want is not None
    assert nt > 0, what


# ------------------------------------------------------------------------------------------- 1. per-window export

@pytest.mark.parametrize("n1p,n2p", POPS)
def test_fixture_holds_every_kind(n1p, n2p):
    SU.assert_kinds(SU.genome(n1p, n2p), n1p, n2p)


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
@pytest.mark.parametrize("n1p,n2p", POPS)
def test_whole_chromosome_records(n1p, n2p, fold):
    """Ranges of 1, 63, 64, 65, 255, 256, 257, 2,047, 2,049 and 9,000 SNPs: the kernel's row and block edges."""
    p = SU.genome(n1p, n2p)
    cfg = _cfg(n1p, n2p, fold=fold, regions=_whole_chroms(p))
    with SU.Run(p, cfg) as r:
        recs, rows = _check_each(p, r.pl, cfg, "whole chromosomes")
    assert (recs["end"] - recs["begin"]).tolist() == SU.LENGTHS
    last = rows[-1][: (2 * n1p + 1) * (2 * n2p + 1)]
    assert last[0] == 0 and last[-1] > 0          # (0, 0) never counted, the last bin counted


@pytest.mark.parametrize("fused", ["0", "1"], ids=["sliced", "fused"])
@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
def test_tiled_and_snp_count_plans(monkeypatch, fold, fused):
    monkeypatch.setenv("SFS2D_FUSED", fused)
    p = SU.genome(12, 12)
    bgs = O.chrom_backgrounds(p, O.Cfg(12, 12, None, fold))
    for kw in ({"window": 20000}, {"window_mode": L.WINDOW_SNPS, "window": 257}):
        cfg = _cfg(fold=fold, **kw)
        with SU.Run(p, cfg) as r:
            v = r.pl.scan_variant()
            assert v["fused"] == int(fused) and v["cnt"] == 1
            recs, rows = _check_each(p, r.pl, cfg, str(kw))
        assert len(recs) > 20
        _check_invariants(p, recs, rows, cfg, lambda c: bgs[c], str(kw))


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
def test_filtered_plan_takes_the_bins(fold):
    """A position filter and variant_type: k_prep's stored bins word (CNT = false)."""
    p = SU.genome(25, 25)
    assert p.ann_names[1] == SU.VT
    bgs = O.chrom_backgrounds(p, O.Cfg(25, 25, SU.VT, fold, FILT["start_position"], FILT["end_position"]))
    for kw in ({"window": 20000}, {"window_mode": L.WINDOW_SNPS, "window": 513}):
        cfg = _cfg(25, 25, fold=fold, **kw, **FILT)
        with SU.Run(p, cfg) as r:
            assert r.pl.scan_variant()["cnt"] == 0
            recs, rows = _check_each(p, r.pl, cfg, f"filtered {kw}")
        unfiltered = SU.expected(p, recs, O.Cfg(25, 25, None, fold))
        assert (rows[:len(recs)] <= unfiltered).all() and rows.sum() < unfiltered.sum()
        _check_invariants(p, recs, rows, cfg, lambda c: bgs[c], f"filtered {kw}")


# ------------------------------------------------------------------------------------------- 2. larger grids

@pytest.mark.parametrize("n1p,n2p,kernel", [(50, 50, "k_scan_gw"), (100, 75, None), (127, 127, None)],
                         ids=["101x101_lds", "201x151_lds_optin", "255x255_global"])
def test_larger_grids(n1p, n2p, kernel):
    """41 KB of LDS, 122 KB (above the default limit: the opt-in), 261 KB (no LDS histogram: global atomics)."""
    p = SU.genome(n1p, n2p, BIG, plant=False)
    for kw in ({"window": 40000}, {"window": 40000, "fold": False, "ann_want": 2}):
        cfg = _cfg(n1p, n2p, **kw)
        with SU.Run(p, cfg) as r:
            if kernel:
                assert r.pl.scan_kernel() == kernel
            recs, rows = _check_each(p, r.pl, cfg, f"{n1p}x{n2p} {kw}")
            pooled = r.pl.spectra(None, np.zeros(len(recs), np.int32), 1)
        assert (recs["end"] - recs["begin"]).max() > 256 and rows.sum() > 1000
        SU.assert_rows(pooled, rows[:len(recs)].sum(axis=0, keepdims=True), "pooled")


# ------------------------------------------------------------------------------------------- 4. partition

@pytest.mark.parametrize("n1p,n2p", POPS)
def test_chromosome_groups_are_the_backgrounds(n1p, n2p):
    """Disjoint tiles partition a chromosome: one group per chromosome is Engine.bg_hist's grid."""
    p = SU.genome(n1p, n2p)
    cfg = _cfg(n1p, n2p, window=200)      # (a few SNPs per window, empty slots between them)
    with SU.Run(p, cfg) as r:
        recs = r.pl.read()
        rows = r.pl.spectra(None, recs["chrom"].astype(np.int32), p.nchrom)
        for c in range(p.nchrom):
            h2, h1a, h1b = r.pl.eng.bg_hist(r.dev, cfg, c)
            g, f1, f2 = SP.split_row(rows[c], n1p, n2p)
            assert np.array_equal(g, h2), c
            assert np.array_equal(f1[1:n1p], O.fold1d(h1a)[1:n1p]) and np.array_equal(f2[1:n2p], O.fold1d(h1b)[1:n2p]), c
            assert f1[0] == f1[n1p] == f2[0] == f2[n2p] == 0
    assert (recs["flags"] & L.W_EMPTY).any()


# ------------------------------------------------------------------------------------------- 5. pooling

def test_pooling():
    p = SU.genome(12, 12)
    cfg = _cfg(window=200)
    ocfg = SU.ocfg_of(cfg, p)
    rng = np.random.default_rng(11)
    with SU.Run(p, cfg) as r:
        recs = r.pl.read()
        empty = np.nonzero(recs["flags"] & L.W_EMPTY)[0]
        live = np.nonzero((recs["flags"] & L.W_EMPTY) == 0)[0]
        assert len(empty) > 10 and len(live) > 1500
        # interleaved, unsorted groups; group 3 has no entry; empties in the list; record live[7] three times
        rec = np.concatenate([rng.choice(live, 300), empty[:10], [live[7]] * 3, rng.choice(len(recs), 200)])
        grp = np.concatenate([rng.integers(0, 3, 300), rng.integers(0, 3, 10), [4, 4, 0], rng.integers(4, 6, 200)])
        order = rng.permutation(len(rec))
        rec, grp = rec[order], grp[order].astype(np.int32)
        got = r.pl.spectra(rec, grp, 6)
        SU.assert_rows(got, SU.expected(p, recs, ocfg, rec, grp, 6), "interleaved")
        assert not got[3].any() and got[0].any()
        # a repeated entry is counted twice
        one = r.pl.spectra([live[7]], [0], 1)
        two = r.pl.spectra([live[7], live[7]], [0, 0], 1)
        assert one.any() and np.array_equal(two, 2 * one)
        # one group of more than 1,000 entries (consecutive entries of one group: one flush per workgroup)
        many = np.sort(rng.choice(len(recs), 1500, replace=False))
        got = r.pl.spectra(many, np.zeros(len(many), np.int32), 2)
        SU.assert_rows(got, SU.expected(p, recs, ocfg, many, np.zeros(len(many), np.int64), 2), "one large group")
        assert not got[1].any()
        # only EMPTY records; no entry at all
        assert not r.pl.spectra(empty[:5], np.zeros(5, np.int32), 1).any()
        z = r.pl.spectra(np.zeros(0, np.int64), np.zeros(0, np.int32), 3)
        assert z.shape == (3, L.spec_row_words(12, 12)) and not z.any()


def test_prev_extra_record_adds_nothing():
    p = SU.genome(12, 12)
    cfg = _cfg(window=20000, prev_extra=True)
    with SU.Run(p, cfg) as r:
        recs, rows = _check_each(p, r.pl, cfg, "prev_extra")
        assert recs[-1]["flags"] & L.W_EXTRA and recs[-1]["end"] > recs[-1]["begin"]     # it has a range of its own
        assert not rows[-1].any() and rows[-2].any()
        k = len(recs) - 1
        assert np.array_equal(r.pl.spectra([k, k - 1], [0, 0], 1)[0], rows[-2])


# ------------------------------------------------------------------------------------------- 6. other plan kinds

def test_sliding_plan():
    p = SU.genome(12, 12)
    cfg = _cfg(window=8000, step=2000)
    with SU.Run(p, cfg) as r:
        recs, rows = _check_each(p, r.pl, cfg, "sliding")
    live = (recs["flags"] & L.W_EMPTY) == 0
    assert live.sum() > 50 and (recs["begin"][live][1:] < recs["end"][live][:-1]).any()      # windows overlap


def test_regions_plan():
    """Overlapping and nested regions, an identical pair, an empty region, a region of more than 2,048 SNPs."""
    from sfs2d.regions import Regions
    p = SU.genome(25, 25)
    c8, c9 = p.chrom_names[8], p.chrom_names[9]
    P9 = p.pos[int(p.chrom_off[9]):].astype(np.int64)
    i = 100 + int(np.argmax(np.diff(P9[100:]) >= 2))
    items = [(c9, 10000, 200000, "outer"), (c9, 50000, 60000, "nested"), (c9, 150000, 300000, "overlapping"),
             (c9, 50000, 60000, "nested_again"), (c9, int(P9[i]) + 1, int(P9[i + 1]) - 1, "empty"),
             (c8, 1, 1 << 31, "chrom8"), (c9, int(P9[2500]), int(P9[2500]), "single")]
    rg = Regions(p.chrom_names, items)
    for filt in ({}, FILT):
        cfg = _cfg(25, 25, regions=rg, **filt)
        with SU.Run(p, cfg) as r:
            recs, rows = _check_each(p, r.pl, cfg, f"regions {filt}")
        by = dict(zip(rg.slot_keys(), range(len(recs))))
        assert recs[by["empty"]]["flags"] & L.W_EMPTY and not rows[by["empty"]].any()
        assert recs[by["outer"]]["end"] - recs[by["outer"]]["begin"] > 2048
        assert np.array_equal(rows[by["nested"]], rows[by["nested_again"]]) and rows[by["nested"]].any()
        assert (rows[by["nested"]] <= rows[by["outer"]]).all()


def test_attached_plans():
    """Attached plans: their own records, the base's data and (filtered) bins."""
    p = SU.genome(12, 12)
    for filt in ({}, FILT):
        base_cfg = _cfg(window=2000, **filt)
        cfgs = [_cfg(window=10000, **filt), _cfg(window_mode=L.WINDOW_SNPS, window=65, **filt),
                _cfg(regions=_whole_chroms(p), **filt)]
        with SU.Run(p, base_cfg, run=False) as r:
            att = [r.pl.attach(c) for c in cfgs]
            with pytest.raises(L.Sfs2dError) as ei:      # an attached plan has no records before its base runs
                att[0].spectra()
            assert ei.value.code == L.E_ARG
            r.pl.run()
            r.pl.check()
            _check_each(p, r.pl, base_cfg, "base")
            for a, c in zip(att, cfgs):
                _check_each(p, a, c, f"attached {c.window_mode} {c.window}")


def test_wrapped_device_data():
    import wide_util as WU
    from sfs2d.engine import Engine
    p = SU.genome(12, 12)
    for filt, ann in (({}, False), (FILT, True)):
        d, keep = WU.wrapped(Engine.get(0), p, ann=ann)
        try:
            for kw in ({"window": 20000}, {"window": 8000, "step": 4000}):
                cfg = _cfg(**kw, **filt)
                with SU.Run(p, cfg, dev=d) as r:
                    _check_each(p, r.pl, cfg, f"wrapped {kw}")
        finally:
            d.close()
        del keep


# ------------------------------------------------------------------------------------------- 7. reproducibility

def test_two_calls_are_byte_equal():
    p = SU.genome(12, 12)
    for cfg in (_cfg(window=20000), _cfg(window_mode=L.WINDOW_SNPS, window=513, ann_want=1)):
        with SU.Run(p, cfg) as r:
            n = r.pl.nrec
            grp = (np.arange(n) % 3).astype(np.int32)
            a, b = r.pl.spectra(), r.pl.spectra()
            c, d = r.pl.spectra(None, grp, 3), r.pl.spectra(None, grp, 3)
            assert a.tobytes() == b.tobytes() and c.tobytes() == d.tobytes() and a.sum() > 0
            assert np.array_equal(c.sum(axis=0), a.sum(axis=0))


@pytest.mark.parametrize("between", [False, True], ids=["spectra", "spectra_div_null_spectra"])
@pytest.mark.parametrize("fused", ["0", "1"], ids=["sliced", "fused"])
def test_following_runs_are_untouched(monkeypatch, fused, between):
    """run, spectra, run (and once more: both replica parities) leaves the later runs' records and Fst byte-equal
    to a plan that never called it; the same with a diversity call and a null run between two spectra calls."""
    monkeypatch.setenv("SFS2D_FUSED", fused)
    p = SU.genome(12, 12)
    cfg = _cfg(window=5000, fst=True, prev_extra=True)
    with SU.Run(p, cfg) as ref:
        assert ref.pl.scan_variant()["fused"] == int(fused)
        want = []
        for _ in range(2):
            ref.pl.run()
            ref.pl.check()
            want.append((ref.pl.read().tobytes(), ref.pl.read_fst().tobytes()))
        div = ref.pl.diversity().tobytes()
    with SU.Run(p, cfg) as r:
        first = None
        for k in range(2):
            s = r.pl.spectra()
            if between:
                assert r.pl.diversity().tobytes() == div
                r.pl.null_run([(0, 1), (9, 513)], 8, 3)
                assert r.pl.spectra().tobytes() == s.tobytes()
                assert r.pl.diversity().tobytes() == div
            first = s if first is None else first
            assert s.tobytes() == first.tobytes()          # the same data, the same windows: every run alike
            r.pl.run()
            r.pl.check()
            assert (r.pl.read().tobytes(), r.pl.read_fst().tobytes()) == want[k], k
        _check_each(p, r.pl, cfg, "after")


def test_caller_buffer():
    import torch
    p = SU.genome(12, 12)
    cfg = _cfg(window=20000)
    with SU.Run(p, cfg) as r:
        want = r.pl.spectra()
        buf = torch.full((want.size + 8,), 7, dtype=torch.int64, device="cuda:0")     # (the call zeroes its rows)
        torch.cuda.synchronize()
        assert r.pl.spectra(out_dev_ptr=buf.data_ptr()) is None
        r.pl.check()                                           # synchronises the engine's stream
        got = buf.cpu().numpy()
        assert np.array_equal(got[:want.size].reshape(want.shape), want) and (got[want.size:] == 7).all()
        n = C.c_int64()      # the read call copies from where the last call wrote
        out = np.zeros(want.shape, np.int64)
        assert r.pl.eng.lib.sfs2d_plan_spectra_read(r.pl.h, L.ptr(out), out.size, C.byref(n)) == 0
        assert n.value == want.size and np.array_equal(out, want)


# ------------------------------------------------------------------------------------------- 8. refusals

def test_refusals():
    p = SU.genome(12, 12)
    cfg = _cfg(window=20000)
    roww = L.spec_row_words(12, 12)
    with SU.Run(p, cfg, run=False) as r:
        lib, h, nrec = r.pl.eng.lib, r.pl.h, r.pl.nrec
        err = lambda: lib.sfs2d_last_error(r.pl.eng.h).decode()
        n = C.c_int64()
        buf = np.zeros(nrec * roww, np.int64)
        i64 = lambda *v: np.array(v, np.int64)
        i32 = lambda *v: np.array(v, np.int32)
        assert lib.sfs2d_plan_spectra(h, None, None, nrec, nrec, None) == L.E_ARG and "first run" in err()
        assert lib.sfs2d_plan_spectra_read(h, L.ptr(buf), buf.size, C.byref(n)) == L.E_ARG     # no call yet
        r.pl.run()
        r.pl.check()
        a, g = i64(0, 1), i32(0, 0)
        assert lib.sfs2d_plan_spectra(h, L.ptr(a), L.ptr(g), -1, 1, None) == L.E_ARG and "nsel" in err()
        assert lib.sfs2d_plan_spectra(h, L.ptr(a), L.ptr(g), 2, 0, None) == L.E_ARG and "ngroups" in err()
        for bad in (i64(0, nrec), i64(-1, 0)):
            assert lib.sfs2d_plan_spectra(h, L.ptr(bad), L.ptr(g), 2, 1, None) == L.E_ARG and "record" in err()
        for bad in (i32(0, 1), i32(-1, 0)):
            assert lib.sfs2d_plan_spectra(h, L.ptr(a), L.ptr(bad), 2, 1, None) == L.E_ARG and "group" in err()
        assert lib.sfs2d_plan_spectra(h, L.ptr(a), None, 2, 2, None) == L.E_ARG and "grp" in err()
        assert lib.sfs2d_plan_spectra(h, None, None, nrec - 1, nrec, None) == L.E_ARG       # NULL rec: nsel == nrec
        assert lib.sfs2d_plan_spectra(h, None, None, nrec, nrec - 1, None) == L.E_ARG       # group i = record i
        # ngroups x row does not fit: the product in 64 bits, and an allocation the device cannot make
        assert lib.sfs2d_plan_spectra(h, L.ptr(a), L.ptr(g), 2, 1 << 62, None) == L.E_NOMEM
        assert lib.sfs2d_plan_spectra(h, L.ptr(a), L.ptr(g), 2, 1 << 31, None) == L.E_NOMEM
        # a good call after the refusals, then the read's capacity
        assert lib.sfs2d_plan_spectra(h, None, None, nrec, nrec, None) == 0
        assert lib.sfs2d_plan_spectra_read(h, L.ptr(buf), buf.size - 1, C.byref(n)) == L.E_CAP
        assert n.value == buf.size
        assert lib.sfs2d_plan_spectra_read(h, L.ptr(buf), buf.size, C.byref(n)) == 0
        SU.assert_rows(buf.reshape(nrec, roww), SU.expected(p, r.pl.read(), SU.ocfg_of(cfg, p)), "after refusals")


# ------------------------------------------------------------------------------------------- 9. class and CLI

def test_class_window_and_outlier_spectra():
    import twoDSFS_class as T
    p = SU.genome(12, 12)
    ocfg = O.Cfg(12, 12)
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=12, pop2_size=12)
    names = p.chrom_names
    wins = {f"{names[c]} {s}-{s + 19999}": (b, e) for c, s, b, e in O.bp_windows(p, 20000)}
    got = obj.window_spectra(p, window_size=20000)
    assert list(got) == list(wins) and len(got) > 20
    for lb, (b, e) in wins.items():
        g, f1, f2 = SP.split_row(SU.oracle_row(p, b, e, ocfg), 12, 12)
        assert np.array_equal(got[lb]["sfs2d"], g) and np.array_equal(got[lb]["sfs1d_pop1"], f1)
        assert np.array_equal(got[lb]["sfs1d_pop2"], f2)
    pick = [list(wins)[5], list(wins)[2]]
    sel = obj.window_spectra(p, window_size=20000, select=pick)
    assert list(sel) == pick and all(np.array_equal(sel[k]["sfs2d"], got[k]["sfs2d"]) for k in pick)
    with pytest.raises(ValueError):
        obj.window_spectra(p, window_size=20000, select=["no such window"])
    snp = obj.window_spectra(p, snp_window_size=300)
    assert list(snp) == list(obj.scan_perChr_bySNPs(p, 300))
    # the outliers: the pooled grid is the numpy twin over select_top's labels
    for kw, key in (({"window_size": 20000}, "T2D"), ({"window_size": 20000, "fst": True}, "FST"),
                    ({"window_size": 8000, "step_size": 2000}, "T2D_diff"), ({"snp_window_size": 300}, "T1D_pop1")):
        res = obj.outlier_spectra(p, key=key, q=0.9, **kw)
        cfg = _cfg(fst=bool(kw.get("fst")), window=kw.get("window_size") or kw["snp_window_size"],
                   step=kw.get("step_size"), window_mode=L.WINDOW_BP if "window_size" in kw else L.WINDOW_SNPS)
        with SU.Run(p, cfg) as r:
            recs = r.pl.read()
            labels = post.record_labels(recs, p, "bp" if "window_size" in kw else "snps", cfg.window, cfg.step)
            rows = obj._clean_rows(recs, labels, r.pl.read_fst() if cfg.fst else None)
        top = SP.select_top(rows, key, 0.9)
        assert res["labels"] == top and 1 <= len(top) < len(rows) / 2
        idx = [labels.index(lb) for lb in top]
        twin = SP.window_spectra_np(p, recs, cfg, idx, np.zeros(len(idx), np.int64), 1)[0]
        assert np.array_equal(res["foreground"], SP.split_row(twin, 12, 12)[0])
        SU.assert_rows(twin[None, :], SU.expected(p, recs, ocfg, idx, np.zeros(len(idx), np.int64), 1), "twin")
        chroms = sorted(set(int(recs[i]["chrom"]) for i in idx))
        assert res["background_chromosomes"] == [names[c] for c in chroms]
        bg = sum(O.sfs2d(p, np.arange(p.chrom_off[c], p.chrom_off[c + 1]), ocfg) for c in chroms)
        assert np.array_equal(res["background"], bg)
        t = res["residuals"]["t2d_term"]
        want = O.clr2d(res["foreground"], bg)
        assert res["T2D"] is not None and abs(res["T2D"] - float(want)) <= 1e-10 * abs(float(want))
        assert abs(math.fsum(t.ravel().tolist()) - float(want)) <= 1e-10 * abs(float(want))
    one = obj.outlier_spectra(p, window_size=20000, q=0.9, background_chromosome=names[9])
    assert one["background_chromosomes"] == [names[9]]
    assert np.array_equal(one["background"], O.sfs2d(p, np.arange(p.chrom_off[9], p.n), ocfg))
    with pytest.raises(ValueError):
        obj.outlier_spectra(p, window_size=20000, key="FST")
    with pytest.raises(NotImplementedError):
        T.LikelihoodInference_jointSFS(None, None, distributed=True).window_spectra(p, window_size=20000)
    with pytest.raises(NotImplementedError):
        T.LikelihoodInference_jointSFS(None, None, distributed=True).outlier_spectra(p, window_size=20000)


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_cli_outputs(tmp_path):
    import twoDSFS_class as T
    from sfs2d import cli
    from sfs2d.vcf import read_vcf
    vcf, pm = os.path.join(GOLD, "vcf_test.vcf.gz"), os.path.join(GOLD, "popmap_3pop.txt")
    p = read_vcf(vcf, pm).to_packed("uv", "bv")
    bed = tmp_path / "genes.bed"
    c0 = p.chrom_names[0]
    P0 = p.pos[:int(p.chrom_off[1])].astype(np.int64)
    bed.write_text(f"{c0}\t{int(P0[10]) - 1}\t{int(P0[60])}\tgeneA\n{c0}\t{int(P0[30]) - 1}\t{int(P0[40])}\tgeneB\n"
                   f"{c0}\t{int(P0[-1]) + 10}\t{int(P0[-1]) + 20}\tempty\n")
    base = [vcf, pm, "--pop1", "uv", "--pop2", "bv", "--pop1-size", "11", "--pop2-size", "11", "--fst",
            "--window", "500000", "--snp-window", "100", "--regions", str(bed)]
    outs = cli.main(base + ["--outlier-spectra", "T2D:0.8", "--outlier-spectra", "FST:0.9", "--region-spectra",
                            "--out-prefix", str(tmp_path / "s")])
    plain = cli.main(base + ["--out-prefix", str(tmp_path / "p")])
    # the old files are byte-identical, and nothing new is written without the new flags
    old = [o for o in outs if os.path.basename(o) in {"s" + os.path.basename(q)[1:] for q in plain}]
    assert len(old) == len(plain) == 3 and [_read(a) for a in old] == [_read(b) for b in plain]
    assert sorted(os.listdir(tmp_path)) == sorted({os.path.basename(x) for x in outs + plain} | {"genes.bed"})
    new = [os.path.basename(o) for o in outs if o not in old]
    stems = [f"s_{size}_{key}_top{pct}" for size in ("500kb", "100snps") for key, pct in (("T2D", "20"), ("FST", "10"))]
    assert sorted(new) == sorted([s + e for s in stems for e in (".fs", "_background.fs", "_residuals.csv")]
                                 + ["s_regions_spectra.npz"])
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=11, pop2_size=11)
    for stem, kw, key, q in ((stems[0], {"window_size": 500000}, "T2D", 0.8),
                             (stems[3], {"snp_window_size": 100, "fst": True}, "FST", 0.9)):
        res = obj.outlier_spectra(p, key=key, q=q, **kw)
        fg, folded, ids, mask = SP.read_dadi_fs(tmp_path / (stem + ".fs"))
        bg = SP.read_dadi_fs(tmp_path / (stem + "_background.fs"))[0]
        assert folded and ids == ("uv", "bv") and mask[0, 0] == mask[-1, -1] == 1 and mask[11, 12] == 1 and mask[11, 11] == 0
        assert fg.dtype == np.int64 and np.array_equal(fg, res["foreground"]) and np.array_equal(bg, res["background"])
        assert fg.sum() > 0
        with open(tmp_path / (stem + "_residuals.csv"), newline="") as fh:
            rows = list(csv.DictReader(fh))
        assert list(rows[0]) == SP.RESIDUAL_COLUMNS and len(rows) == int(((fg != 0) | (bg != 0)).sum())
        for row in rows:
            i, j = int(row["x1"]), int(row["x2"])
            assert int(row["fg_count"]) == fg[i, j] and int(row["bg_count"]) == bg[i, j]
        tsum = math.fsum(float(row["t2d_term"]) for row in rows)
        want = float(O.clr2d(fg, bg))
        assert abs(tsum - want) <= 1e-10 * abs(want) and abs(res["T2D"] - want) <= 1e-10 * abs(want)
    z = np.load(tmp_path / "s_regions_spectra.npz")
    assert z["name"].tolist() == ["geneA", "geneB", "empty"] and z["sfs2d"].shape == (3, 23, 23)
    ocfg = O.Cfg(11, 11)
    for k, (b, e) in enumerate(((10, 61), (30, 41), (0, 0))):
        g, f1, f2 = SP.split_row(SU.oracle_row(p, b, e, ocfg), 11, 11)
        assert np.array_equal(z["sfs2d"][k], g) and np.array_equal(z["sfs1d_pop1"][k], f1)
        assert np.array_equal(z["sfs1d_pop2"][k], f2)
    assert z["sfs2d"][0].sum() > 0 and not z["sfs2d"][2].any()
