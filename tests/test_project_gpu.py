"""Projected window spectra on the device (kernel k_proj_win, sfs2d_plan_project) against the
exact twin sfs2d.spectra.project_np (tests/project_util.py): n_used / n_dropped exact, every grid bin within
K_g 2^-(e + 1) + 2 R value (one rounding per term at 2^-e, K_g the group's used SNPs; R four times the weights' worst
relative error, measured on the host), the anchor -- full-size projection of fully called data -- exact integers.

The genome is spectra_util's (chromosomes of 1 .. 9,000 SNPs, pop 18 / 14, 2 % missing alleles) with the projection's
awkward SNPs planted at the row edges (project_util.planted); test_project_cpu.py asserts the fixtures' properties on
the twin.  (36, 28) runs on the fully called copy: with 2 % missing alleles half the SNPs miss the full size.  The
large grids (100 / 75 at (160, 120): a 156 kB row, the opt-in LDS path; 127 / 127 at (254, 254), fully called: 520 kB,
global atomics) run at ~3,300 SNPs."""
import ctypes as C
import os

import numpy as np
import pytest

import project_util as PU
import spectra_util as SU
from golden_util import GOLD
from sfs2d import _lib as L
from sfs2d import post
from sfs2d import spectra as SP

pytestmark = pytest.mark.gpu

N1P, N2P = 18, 14
M = (24, 20)
SHAPES = [((2, 2), False), ((7, 5), False), ((24, 20), False), ((36, 28), True)]
BIG = [2049, 1000, 257]
FILT = {"start_position": 3000, "end_position": 400000, "ann_want": 1}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE", "SFS2D_SLOTS_ONCE"):
        monkeypatch.delenv(k, raising=False)


def _cfg(n1p=N1P, n2p=N2P, **kw):
    from sfs2d.engine import ScanConfig
    return ScanConfig(n1p=n1p, n2p=n2p, **kw)


def _whole_chroms(p):
    from sfs2d.regions import Regions
    return Regions(p.chrom_names, [(c, 0, (1 << 32) - 1, f"whole_{c}") for c in p.chrom_names])


def _check_each(p, pl, cfg, m, what=""):
    """Per-window projection (rec = NULL, group i = record i) against the twin; returns (records, grids, used)."""
    recs = pl.read()
    g, u, d = pl.project(*m)
    assert g.shape == (max(1, pl.nrec), m[0] + 1, m[1] + 1)
    n = len(recs)
    PU.assert_grids(g[:n], u[:n], d[:n], PU.twin(p, recs, cfg, *m), pl.project_e, what)
    live = (recs["flags"] & (L.W_EMPTY | L.W_EXTRA)) == 0
    assert np.array_equal((u[:n] + d[:n])[live], recs["n2_all"][live].astype(np.int64)), what    # the scan's own members
    assert not g[:n][~live].any() and not u[:n][~live].any() and not d[:n][~live].any()
    return recs, g, u


# ------------------------------------------------------------------------------------------- 1. shapes

@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
@pytest.mark.parametrize("m,full", SHAPES, ids=[f"{a}x{b}" for (a, b), _ in SHAPES])
def test_whole_chromosome_records(m, full, fold):
    """Ranges of 1, 63, 64, 65, 255, 256, 257, 2,047, 2,049 and 9,000 SNPs: the kernel's row and block edges.  The
    plan's fold decides membership alone; the grid is unfolded either way."""
    p = PU.genome(N1P, N2P, m, full=full)
    cfg = _cfg(fold=fold, regions=_whole_chroms(p))
    with SU.Run(p, cfg) as r:
        recs, g, u = _check_each(p, r.pl, cfg, m, f"whole chromosomes {m}")
        assert r.pl.project_e == 40                      # one entry of at most 9,000 SNPs per group
        # the chromosome entries: the same ranges, named by chromosome
        ch = r.pl.project(*m, [-(c + 1) for c in range(p.nchrom)], np.arange(p.nchrom, dtype=np.int32), p.nchrom)
        assert all(np.array_equal(a, b) for a, b in zip(ch, (g, u, r.pl.project(*m)[2])))
    assert (recs["end"] - recs["begin"]).tolist() == SU.LENGTHS and u[-1] > 7000
    assert g[-1][0, 0] > 0 or m == (36, 28)              # (SNPs that project to no alt copy at all stay in (0, 0))


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
def test_anchor_full_size_on_fully_called_data(fold):
    """m = (36, 28) on data without missing or surplus calls: every weight is exactly 1, so the folded grid times 2^e
    is sfs2d_plan_spectra's integer grid, and the marginals' folds at the inner bins are its 1D spectra."""
    p = PU.genome(N1P, N2P, None, full=True)
    assert (p.ref1.astype(int) + p.alt1 == 2 * N1P).all() and (p.ref2.astype(int) + p.alt2 == 2 * N2P).all()
    for kw in ({"regions": _whole_chroms(p)}, {"window": 20000}):
        cfg = _cfg(fold=fold, **kw)
        with SU.Run(p, cfg) as r:
            rows = r.pl.spectra()
            g, u, d = r.pl.project(2 * N1P, 2 * N2P)
            e = r.pl.project_e
        assert not d.any() and u.sum() > 10000
        for k in range(len(rows)):
            grid, f1, f2 = SP.split_row(rows[k], N1P, N2P)
            scaled = np.ldexp(SP.fold_projected(g[k]) if fold else g[k], e)
            assert np.array_equal(scaled, grid.astype(np.float64) * 2.0 ** e), k
            assert u[k] == grid.sum()
            s1, s2 = SP.projected_marginals(g[k])
            assert np.array_equal(SP.fold1d_projected(s1)[1:N1P], f1[1:N1P].astype(np.float64)), k
            assert np.array_equal(SP.fold1d_projected(s2)[1:N2P], f2[1:N2P].astype(np.float64)), k


@pytest.mark.parametrize("n1p,n2p,m,full", [(100, 75, (160, 120), False), (127, 127, (254, 254), True)],
                         ids=["161x121_lds_optin", "255x255_global"])
def test_larger_grids(n1p, n2p, m, full):
    """A 156 kB row (above the default LDS limit: the opt-in) and a 520 kB row (no LDS histogram: global atomics)."""
    p = PU.genome(n1p, n2p, m, lengths=BIG, full=full)
    cfg = _cfg(n1p, n2p, regions=_whole_chroms(p))
    with SU.Run(p, cfg) as r:
        recs, g, u = _check_each(p, r.pl, cfg, m, f"{m}")
        pooled = r.pl.project(*m, None, np.zeros(len(recs), np.int32), 1)
    assert u.sum() > 2500
    PU.assert_grids(*pooled, PU.twin(p, recs, cfg, *m, None, np.zeros(len(recs), np.int64), 1), r.pl.project_e, "pooled")


# ------------------------------------------------------------------------------------------- 2. plan kinds

@pytest.mark.parametrize("fused", ["0", "1"], ids=["sliced", "fused"])
def test_tiled_and_snp_count_plans(monkeypatch, fused):
    monkeypatch.setenv("SFS2D_FUSED", fused)
    p = PU.genome(N1P, N2P, M)
    for kw in ({"window": 20000}, {"window_mode": L.WINDOW_SNPS, "window": 257}):
        cfg = _cfg(**kw)
        with SU.Run(p, cfg) as r:
            v = r.pl.scan_variant()
            assert v["fused"] == int(fused) and v["cnt"] == 1
            recs, g, u = _check_each(p, r.pl, cfg, M, str(kw))
        assert len(recs) > 20 and u.sum() > 10000


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
def test_filtered_plan_takes_the_bins(fold):
    """A position filter and variant_type: membership from k_prep's stored bins word (CNT = false), 8 B/SNP."""
    p = PU.genome(N1P, N2P, M)
    assert p.ann_names[1] == SU.VT
    for kw, m in (({"window": 20000}, M), ({"window_mode": L.WINDOW_SNPS, "window": 513}, (7, 5))):
        q = p if m == M else PU.genome(N1P, N2P, m)
        cfg = _cfg(fold=fold, **kw, **FILT)
        with SU.Run(q, cfg) as r:
            assert r.pl.scan_variant()["cnt"] == 0
            recs, g, u = _check_each(q, r.pl, cfg, m, f"filtered {kw}")
        free = PU.twin(q, recs, _cfg(fold=fold, **kw), *m)
        assert 0 < u.sum() < free[1].sum() / 2


def test_sliding_plan_and_chromosome_entries():
    p = PU.genome(N1P, N2P, M)
    cfg = _cfg(window=8000, step=2000)
    with SU.Run(p, cfg) as r:
        recs, g, u = _check_each(p, r.pl, cfg, M, "sliding")
        rec = [-(c + 1) for c in range(p.nchrom)] + [-10, -10]
        grp = list(range(p.nchrom)) + [9, 0]
        got = r.pl.project(*M, rec, grp, p.nchrom)
        PU.assert_grids(*got, PU.twin(p, recs, cfg, *M, rec, grp, p.nchrom), r.pl.project_e, "chromosome entries")
        assert r.pl.project_e == 40          # two entries of up to 9,000 SNPs: B = 18,000, 15 bits
    live = (recs["flags"] & L.W_EMPTY) == 0
    assert live.sum() > 50 and (recs["begin"][live][1:] < recs["end"][live][:-1]).any()      # windows overlap


def test_regions_plan():
    """Overlapping and nested regions, an identical pair, an empty region, a region of more than 2,048 SNPs."""
    from sfs2d.regions import Regions
    p = PU.genome(N1P, N2P, M)
    c8, c9 = p.chrom_names[8], p.chrom_names[9]
    P9 = p.pos[int(p.chrom_off[9]):].astype(np.int64)
    i = 100 + int(np.argmax(np.diff(P9[100:]) >= 2))
    items = [(c9, 10000, 200000, "outer"), (c9, 50000, 60000, "nested"), (c9, 150000, 300000, "overlapping"),
             (c9, 50000, 60000, "nested_again"), (c9, int(P9[i]) + 1, int(P9[i + 1]) - 1, "empty"),
             (c8, 1, 1 << 31, "chrom8"), (c9, int(P9[2500]), int(P9[2500]), "single")]
    rg = Regions(p.chrom_names, items)
    for filt in ({}, FILT):
        cfg = _cfg(regions=rg, **filt)
        with SU.Run(p, cfg) as r:
            recs, g, u = _check_each(p, r.pl, cfg, M, f"regions {filt}")
        by = dict(zip(rg.slot_keys(), range(len(recs))))
        assert recs[by["empty"]]["flags"] & L.W_EMPTY and not g[by["empty"]].any()
        assert recs[by["outer"]]["end"] - recs[by["outer"]]["begin"] > 2048
        assert np.array_equal(g[by["nested"]], g[by["nested_again"]]) and g[by["nested"]].any()


def test_attached_plans():
    p = PU.genome(N1P, N2P, M)
    for filt in ({}, FILT):
        base_cfg = _cfg(window=2000, **filt)
        cfgs = [_cfg(window=10000, **filt), _cfg(window_mode=L.WINDOW_SNPS, window=65, **filt),
                _cfg(regions=_whole_chroms(p), **filt)]
        with SU.Run(p, base_cfg, run=False) as r:
            att = [r.pl.attach(c) for c in cfgs]
            with pytest.raises(L.Sfs2dError) as ei:      # an attached plan has no records before its base runs
                att[0].project(*M)
            assert ei.value.code == L.E_ARG
            r.pl.run()
            r.pl.check()
            _check_each(p, r.pl, base_cfg, M, "base")
            for a, c in zip(att, cfgs):
                _check_each(p, a, c, M, f"attached {c.window_mode} {c.window}")


def test_wrapped_device_data():
    import wide_util as WU
    from sfs2d.engine import Engine
    p = PU.genome(N1P, N2P, M)
    for filt, ann in (({}, False), (FILT, True)):
        d, keep = WU.wrapped(Engine.get(0), p, ann=ann)
        try:
            for kw in ({"window": 20000}, {"window": 8000, "step": 4000}):
                cfg = _cfg(**kw, **filt)
                with SU.Run(p, cfg, dev=d) as r:
                    _check_each(p, r.pl, cfg, M, f"wrapped {kw}")
        finally:
            d.close()
        del keep


# ------------------------------------------------------------------------------------------- 3. pooling

def test_pooling_and_the_fixed_point():
    p = PU.genome(N1P, N2P, M)
    cfg = _cfg(window=200)      # (a few SNPs per window, empty slots between them)
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
        got = r.pl.project(*M, rec, grp, 6)
        PU.assert_grids(*got, PU.twin(p, recs, cfg, *M, rec, grp, 6), r.pl.project_e, "interleaved")
        assert not got[0][3].any() and got[0][0].any() and got[1][3] == got[2][3] == 0
        # a repeated entry is counted twice: the same rounded terms, twice
        one, two = r.pl.project(*M, [live[7]], [0], 1), r.pl.project(*M, [live[7], live[7]], [0, 0], 1)
        assert one[0].any() and all(np.array_equal(b, 2 * a) for a, b in zip(one, two))
        # only EMPTY records; no entry at all
        z = r.pl.project(*M, empty[:5], np.zeros(5, np.int32), 1)
        assert not z[0].any() and not z[1].any() and not z[2].any()
        z = r.pl.project(*M, np.zeros(0, np.int64), np.zeros(0, np.int32), 3)
        assert z[0].shape == (3, M[0] + 1, M[1] + 1) and not z[0].any() and not z[1].any()
    # the EXTRA record adds nothing
    cfg = _cfg(window=20000, prev_extra=True)
    with SU.Run(p, cfg) as r:
        recs, g, u = _check_each(p, r.pl, cfg, M, "prev_extra")
        assert recs[-1]["flags"] & L.W_EXTRA and recs[-1]["end"] > recs[-1]["begin"] and not g[-1].any() and g[-2].any()
    # one group of 1,500 entries over whole-chromosome records: B = 1,500 x 9,000 < 2^24, e = 62 - 24
    cfg = _cfg(regions=_whole_chroms(p))
    with SU.Run(p, cfg) as r:
        recs = r.pl.read()
        many = rng.integers(0, len(recs), 1500)
        grp = np.zeros(1500, np.int32)
        grp[7] = 1                       # (and one entry beside it: e is set by the largest group)
        got = r.pl.project(*M, many, grp, 2)
        assert r.pl.project_e == 38
        PU.assert_grids(*got, PU.twin(p, recs, cfg, *M, many, grp, 2), 38, "one large group")
        assert got[1][0] > 1000000
        r.pl.project(*M)
        assert r.pl.project_e == 40      # one entry per group: min(40, 62 - bitlen(9,000))


# ------------------------------------------------------------------------------------------- 4. reproducibility

def test_two_calls_are_byte_equal():
    p = PU.genome(N1P, N2P, M)
    for cfg in (_cfg(window=20000), _cfg(window_mode=L.WINDOW_SNPS, window=513, ann_want=1)):
        with SU.Run(p, cfg) as r:
            n = r.pl.nrec
            grp = (np.arange(n) % 3).astype(np.int32)
            a, b = r.pl.project(*M), r.pl.project(*M)
            c, d = r.pl.project(*M, None, grp, 3), r.pl.project(*M, None, grp, 3)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a + c, b + d)) and a[0].sum() > 0
            # (integer sums of the same rounded terms: pooling is exact)
            assert np.array_equal(c[0].sum(axis=0), a[0].sum(axis=0)) and c[1].sum() == a[1].sum()


@pytest.mark.parametrize("fused", ["0", "1"], ids=["sliced", "fused"])
def test_following_runs_are_untouched(monkeypatch, fused):
    """run, project, run (and once more: both replica parities) leaves the later runs' records and Fst byte-equal to
    a plan that never called it, with a spectra, a diversity and a null call in between, which see what they saw."""
    monkeypatch.setenv("SFS2D_FUSED", fused)
    p = PU.genome(N1P, N2P, M)
    cfg = _cfg(window=5000, fst=True, prev_extra=True)
    with SU.Run(p, cfg) as ref:
        assert ref.pl.scan_variant()["fused"] == int(fused)
        want = []
        for _ in range(2):
            ref.pl.run()
            ref.pl.check()
            want.append((ref.pl.read().tobytes(), ref.pl.read_fst().tobytes()))
        div, spec = ref.pl.diversity().tobytes(), ref.pl.spectra().tobytes()
        ref.pl.null_run([(0, 1), (9, 513)], 8, 3)
        null = ref.pl.null_read().tobytes()
    with SU.Run(p, cfg) as r:
        first = None
        for k in range(2):
            s = r.pl.project(*M)
            assert r.pl.spectra().tobytes() == spec and r.pl.diversity().tobytes() == div
            r.pl.null_run([(0, 1), (9, 513)], 8, 3)
            assert r.pl.null_read().tobytes() == null
            t = r.pl.project(*M)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(s, t))
            first = s if first is None else first
            assert all(x.tobytes() == y.tobytes() for x, y in zip(s, first))      # every run alike
            r.pl.run()
            r.pl.check()
            assert (r.pl.read().tobytes(), r.pl.read_fst().tobytes()) == want[k], k
        _check_each(p, r.pl, cfg, M, "after")


def test_caller_buffer():
    import torch
    p = PU.genome(N1P, N2P, M)
    cfg = _cfg(window=20000)
    roww = L.proj_row_words(*M)
    with SU.Run(p, cfg) as r:
        g, u, d = r.pl.project(*M)
        e = r.pl.project_e
        buf = torch.full((len(g) * roww + 8,), 7, dtype=torch.int64, device="cuda:0")     # (the call zeroes its rows)
        torch.cuda.synchronize()
        assert r.pl.project(*M, out_dev_ptr=buf.data_ptr()) is None and r.pl.project_e == e
        r.pl.check()                                           # synchronises the engine's stream
        got = buf.cpu().numpy()
        rows = got[:len(g) * roww].reshape(len(g), roww)
        assert (got[len(g) * roww:] == 7).all()
        assert np.array_equal(rows[:, :-2].astype(np.float64) * 2.0 ** -e, g.reshape(len(g), -1))
        assert np.array_equal(rows[:, -2], u) and np.array_equal(rows[:, -1], d)
        # the read call copies from where the last call wrote
        out, uu, dd = np.zeros_like(g), np.zeros_like(u), np.zeros_like(d)
        n, w = C.c_int64(), C.c_int64()
        assert r.pl.eng.lib.sfs2d_plan_project_read(r.pl.h, L.ptr(out), L.ptr(uu), L.ptr(dd), len(g), C.byref(n),
                                                    C.byref(w)) == 0
        assert (n.value, w.value) == (len(g), roww - 2) and np.array_equal(out, g) and np.array_equal(uu, u)


# ------------------------------------------------------------------------------------------- 5. refusals

def test_refusals():
    p = PU.genome(N1P, N2P, M)
    cfg = _cfg(window=20000)
    with SU.Run(p, cfg, run=False) as r:
        lib, h, nrec = r.pl.eng.lib, r.pl.h, r.pl.nrec
        err = lambda: lib.sfs2d_last_error(r.pl.eng.h).decode()
        n, w, e = C.c_int64(), C.c_int64(), C.c_int32()
        out, uu, dd = np.zeros((nrec, 25, 21)), np.zeros(nrec, np.int64), np.zeros(nrec, np.int64)
        i64 = lambda *v: np.array(v, np.int64)
        i32 = lambda *v: np.array(v, np.int32)
        call = lambda m1, m2, rec, grp, nsel, ng: lib.sfs2d_plan_project(h, m1, m2, L.ptr(rec), L.ptr(grp), nsel, ng, None,
                                                                         C.byref(e))
        read = lambda cap: lib.sfs2d_plan_project_read(h, L.ptr(out), L.ptr(uu), L.ptr(dd), cap, C.byref(n), C.byref(w))
        assert call(24, 20, None, None, nrec, nrec) == L.E_ARG and "first run" in err()
        assert read(nrec) == L.E_ARG                                                       # no call yet
        r.pl.run()
        r.pl.check()
        a, g = i64(0, 1), i32(0, 0)
        for m1, m2 in ((1, 20), (37, 20), (24, 1), (24, 29), (0, 0), (-3, 20)):
            assert call(m1, m2, a, g, 2, 1) == L.E_ARG and "outside [2, 36] x [2, 28]" in err(), (m1, m2)
        assert call(24, 20, a, g, -1, 1) == L.E_ARG and "nsel" in err()
        assert call(24, 20, a, g, 2, 0) == L.E_ARG and "ngroups" in err()
        assert call(24, 20, i64(0, nrec), g, 2, 1) == L.E_ARG and "record" in err()
        for bad in (i64(0, -(p.nchrom + 1)), i64(-(1 << 40), 0)):
            assert call(24, 20, bad, g, 2, 1) == L.E_ARG and "chromosome" in err()
        for bad in (i32(0, 1), i32(-1, 0)):
            assert call(24, 20, a, bad, 2, 1) == L.E_ARG and "group" in err()
        assert call(24, 20, a, None, 2, 2) == L.E_ARG and "grp" in err()
        assert call(24, 20, None, None, nrec - 1, nrec) == L.E_ARG       # NULL rec: nsel == nrec
        assert call(24, 20, None, None, nrec, nrec - 1) == L.E_ARG       # group i = record i
        # ngroups x row does not fit: the product in 64 bits, and an allocation the device cannot make
        assert call(24, 20, a, g, 2, 1 << 62) == L.E_NOMEM
        assert call(24, 20, a, g, 2, 1 << 31) == L.E_NOMEM
        # a good call after the refusals (the last chromosome among the entries), then the read's capacity
        assert call(24, 20, i64(0, -p.nchrom), i32(0, 1), 2, nrec) == 0 and e.value == 40
        assert read(nrec - 1) == L.E_CAP and (n.value, w.value) == (nrec, 25 * 21)
        assert read(nrec) == 0
        want = PU.twin(p, r.pl.read(), cfg, 24, 20, [0, -p.nchrom], [0, 1], nrec)
        PU.assert_grids(out, uu, dd, want, 40, "after refusals")


# ------------------------------------------------------------------------------------------- 6. class and CLI

def test_class_window_and_outlier_spectra():
    import twoDSFS_class as T
    p = PU.genome(N1P, N2P, M)
    names = p.chrom_names
    for fold in (True, False):
        obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=N1P, pop2_size=N2P, fold=fold)
        cfg = _cfg(window=20000, fold=fold)
        with SU.Run(p, cfg) as r:
            recs = r.pl.read()
            labels = post.record_labels(recs, p, "bp", 20000, None)
            g, u, d = r.pl.project(*M)
            e = r.pl.project_e
        got = obj.window_spectra(p, window_size=20000, project=M)
        keep = [i for i, lb in enumerate(labels) if lb is not None]
        assert list(got) == [labels[i] for i in keep] and len(got) > 20
        for i in keep:
            w = got[labels[i]]
            want = SP.fold_projected(g[i]) if fold else g[i]
            s1, s2 = SP.projected_marginals(g[i])
            assert np.array_equal(w["sfs2d"], want) and (w["n_used"], w["n_dropped"]) == (u[i], d[i])
            assert np.array_equal(w["sfs1d_pop1"], SP.fold1d_projected(s1) if fold else s1)
            assert np.array_equal(w["sfs1d_pop2"], SP.fold1d_projected(s2) if fold else s2)
        pick = [labels[keep[5]], labels[keep[2]]]
        sel = obj.window_spectra(p, window_size=20000, select=pick, project=M)
        assert list(sel) == pick and all(np.array_equal(sel[k]["sfs2d"], got[k]["sfs2d"]) for k in pick)
        # the outliers: foreground and background both projected, against the twin
        for kw, key in (({"window_size": 20000}, "T2D"), ({"window_size": 8000, "step_size": 2000}, "T2D_diff")):
            res = obj.outlier_spectra(p, key=key, q=0.9, project=M, **kw)
            plain = obj.outlier_spectra(p, key=key, q=0.9, **kw)
            assert res["labels"] == plain["labels"] and res["background_chromosomes"] == plain["background_chromosomes"]
            c2 = _cfg(window=kw["window_size"], step=kw.get("step_size"), fold=fold)
            with SU.Run(p, c2) as r:
                recs2 = r.pl.read()
            lab2 = post.record_labels(recs2, p, "bp", c2.window, c2.step)
            idx = [lab2.index(lb) for lb in res["labels"]]
            chroms = [names.index(c) for c in res["background_chromosomes"]]
            rec = idx + [-(c + 1) for c in chroms]
            grp = [0] * len(idx) + [1] * len(chroms)
            tg, tu, td = PU.twin(p, recs2, c2, *M, rec, grp, 2)
            # (no entry holds more SNPs than the longest chromosome, 9,000: the call's e is at least this)
            e_lo = PU.fixed_point_e(max(len(idx), len(chroms)), 9000)
            PU.assert_folded(np.stack([res["foreground"], res["background"]]), tg, tu, e_lo, fold, key)
            assert (res["n_used"], res["n_dropped"], res["background_n_used"], res["background_n_dropped"]) == \
                (tu[0], td[0], tu[1], td[1])
            assert res["T2D"] == SP.pooled_t2d(SP.residuals(res["foreground"], res["background"]))
            assert res["T2D"] is not None and res["T2D"] > 0
        one = obj.outlier_spectra(p, window_size=20000, q=0.9, background_chromosome=names[9], project=M)
        assert one["background_chromosomes"] == [names[9]] and one["background_n_used"] > 7000


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_cli_outputs(tmp_path, capsys):
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
    base = [vcf, pm, "--pop1", "uv", "--pop2", "bv", "--pop1-size", "11", "--pop2-size", "11", "--window", "500000",
            "--regions", str(bed), "--outlier-spectra", "T2D:0.8", "--region-spectra"]
    plain = cli.main(base + ["--out-prefix", str(tmp_path / "p")])
    capsys.readouterr()
    outs = cli.main(base + ["--project", "16,14", "--out-prefix", str(tmp_path / "s")])
    errtext = capsys.readouterr().err
    # without --project every file is what it was; with it the scans' files are, and the spectra files are renamed
    names = lambda paths, pre: sorted(os.path.basename(x)[len(pre):] for x in paths)
    assert not any("_proj" in n for n in names(plain, "p"))
    assert names(outs, "s") == sorted(n.replace("_top20", "_top20_proj16x14").replace("_spectra.npz", "_spectra_proj16x14.npz")
                                      for n in names(plain, "p"))
    for a in plain:
        if a.endswith(".csv") and "residuals" not in a:
            assert _read(a) == _read(str(tmp_path / ("s" + os.path.basename(a)[1:])))
    assert errtext.count("SNPs dropped (") == 3 and "projection (16, 14)" in errtext
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=11, pop2_size=11)
    res = obj.outlier_spectra(p, key="T2D", q=0.8, window_size=500000, project=(16, 14))
    stem = "s_500kb_T2D_top20_proj16x14"
    fg, folded, ids, mask = SP.read_dadi_fs(tmp_path / (stem + ".fs"))
    bg = SP.read_dadi_fs(tmp_path / (stem + "_background.fs"))[0]
    assert folded and ids == ("uv", "bv") and fg.shape == (17, 15) and mask[0, 0] == mask[-1, -1] == 1 and mask[8, 8] == 1
    assert fg.dtype == np.float64 and np.array_equal(fg, res["foreground"]) and np.array_equal(bg, res["background"])
    assert 0 < res["n_used"]
    import csv
    with open(tmp_path / (stem + "_residuals.csv"), newline="") as fh:
        rows = list(csv.DictReader(fh))
    assert len(rows) == int(((fg != 0) | (bg != 0)).sum())
    for row in rows:
        i, j = int(row["x1"]), int(row["x2"])
        assert float(row["fg_count"]) == fg[i, j] and float(row["bg_count"]) == bg[i, j]
    z = np.load(tmp_path / "s_regions_spectra_proj16x14.npz")
    assert z["name"].tolist() == ["geneA", "geneB", "empty"] and z["sfs2d"].shape == (3, 17, 15)
    assert z["sfs1d_pop1"].shape == (3, 17) and z["sfs1d_pop2"].shape == (3, 15)
    recs = np.zeros(3, L.WINDOW_DTYPE)
    recs["begin"], recs["end"] = [10, 30, 0], [61, 41, 0]
    tg, tu, td = SP.project_np(p, recs, PU.Cfg(11, 11), 16, 14)
    assert z["n_used"].tolist() == tu.tolist() and z["n_dropped"].tolist() == td.tolist() and tu[0] > 0 and tu[2] == 0
    PU.assert_folded(z["sfs2d"], tg, tu, 40, True, "regions npz")      # (one entry of a few SNPs per group: e = 40)
    assert not z["sfs2d"][2].any()
