"""The projected scan on the device (kernels k_proj_lp and k_proj_scan, sfs2d_plan_project_scan),
checked three ways per record (tests/projscan_util.py):

* the integer link, exact: n_used, n_dropped and the three N as fixed-point integers against ``Plan.project``'s own grid
  of the record, at the same exponent e;
* the device's arithmetic: the closed form evaluated in float64 on the host from ``Plan.project``'s window and
  chromosome-entry grids, within 1e-10 A, A = sum |x_k ln(x_k / N)| + |x_k lp_k| (an fp64 sum of at most (m1 + 1)(m2 + 1)
  terms of a few ulp each stays below 2e-12 A); +inf and NaN at the same records;
* everything, against the exact twin sfs2d.spectra.project_scan_np: |dT| <= 2 x the first-order bound + 1e-10 A.

``_check`` prints the worst err / A and err / bound it saw (``-s``); DESIGN.md section 19 records them.

The genome is project_util's 14,000-SNP one (18 / 14, 2 % missing alleles) with an all-dropped 3-SNP window planted;
test_project_scan_cpu.py asserts the fixtures' properties on the twin."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import project_util as PU
import projscan_util as PS
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
FIELDS = ("t2d", "t1d_p1", "t1d_p2")
WORST = {"arith": 0.0, "twin": 0.0}


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


def _check(p, pl, cfg, m, bg_chrom=None, what="", exact=True, twin=True):
    """One project_scan call of a plan that has run, checked the three ways of the module docstring; returns
    (records, stats)."""
    recs = pl.read()
    st = pl.project_scan(*m, bg_chrom)
    e, e_bg = pl.project_scan_e, pl.project_scan_e_bg
    assert st.dtype == L.PROJSTAT_DTYPE and len(st) == len(recs)
    g, u, d = pl.project(*m)
    assert pl.project_e == e, (what, pl.project_e, e)                       # one record per group: the same exponent
    chroms = list(range(p.nchrom)) if bg_chrom is None else [bg_chrom]
    gb, ub, _ = pl.project(*m, [-(c + 1) for c in chroms], np.arange(len(chroms), dtype=np.int32), len(chroms))
    assert pl.project_e == e_bg, (what, pl.project_e, e_bg)                 # one chromosome entry per group
    tw = None
    if twin:
        tw = PS.twin(p, recs, cfg, *m, bg_chrom) if exact else SP.project_scan_np(p, recs, cfg, *m, bg_chrom)
    dead = (recs["flags"] & (L.W_EMPTY | L.W_EXTRA)) != 0
    assert np.array_equal(st["flags"], recs["flags"] & (L.W_EMPTY | L.W_EXTRA)), what
    for f in st.dtype.names:
        if f != "flags":
            assert not st[f][dead].any(), (what, f)
    worst_a = worst_t = 0.0
    for i in np.nonzero(~dead)[0].tolist():
        s = st[i]
        assert (int(s["n_used"]), int(s["n_dropped"]), int(s["e"])) == (int(u[i]), int(d[i]), e), (what, i)
        assert (int(s["n2_fx"]), int(s["n1a_fx"]), int(s["n1b_fx"])) == PS.fixed_sums(g[i], cfg.fold, e), (what, i)
        c = 0 if bg_chrom is not None else int(recs[i]["chrom"])
        ref = PS.closed_form(g[i], gb[c], cfg.fold, int(u[i]), int(ub[c]), e, e_bg)
        for f, (T, A, bound) in zip(FIELDS, ref):
            got = float(s[f])
            if math.isnan(T) or math.isinf(T):
                assert (math.isnan(got) and math.isnan(T)) or got == T, (what, i, f, got, T)
            else:
                assert math.isfinite(got) and abs(got - T) <= 1e-10 * A, (what, i, f, got, T, A)
                if A > 0:
                    worst_a = max(worst_a, abs(got - T) / A)
            if tw is not None:
                W = float(tw[f][i])
                if math.isnan(W) or math.isinf(W):
                    assert (math.isnan(got) and math.isnan(W)) or got == W, (what, i, f, got, W)
                else:
                    assert math.isfinite(got) and abs(got - W) <= 2.0 * bound + 1e-10 * A, (what, i, f, got, W, bound, A)
                    if bound > 0:
                        worst_t = max(worst_t, abs(got - W) / bound)
    if tw is not None:
        assert np.array_equal(st["n_used"], tw["n_used"]) and np.array_equal(st["n_dropped"], tw["n_dropped"]), what
    WORST["arith"], WORST["twin"] = max(WORST["arith"], worst_a), max(WORST["twin"], worst_t)
    print(f"{what}: {int((~dead).sum())} records, e {e} / {e_bg}, worst err / A {worst_a:.3g}, worst err / bound "
          f"{worst_t:.3g} (file so far {WORST['arith']:.3g}, {WORST['twin']:.3g})")
    return recs, st


# ------------------------------------------------------------------------------------------- 1. shapes

@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
@pytest.mark.parametrize("m,full", SHAPES, ids=[f"{a}x{b}" for (a, b), _ in SHAPES])
def test_whole_chromosome_records(m, full, fold):
    """Records of 1, 63, 64, 65, 255, 256, 257, 2,047, 2,049 and 9,000 SNPs (the row and block edges), each against its
    own chromosome -- itself: T = 0 to rounding -- and all against the longest."""
    p = PS.genome(N1P, N2P, m, full=full)
    cfg = _cfg(fold=fold, regions=_whole_chroms(p))
    with SU.Run(p, cfg) as r:
        recs, st = _check(p, r.pl, cfg, m, None, f"whole chromosomes {m} own")
        assert r.pl.project_scan_e == r.pl.project_scan_e_bg == 40
        recs, long_ = _check(p, r.pl, cfg, m, 9, f"whole chromosomes {m} against the longest")
    assert (recs["end"] - recs["begin"]).tolist() == SU.LENGTHS
    assert st["n_used"][-1] > 7000 and np.isfinite(st["t2d"][4:]).all() and (np.abs(st["t2d"][4:]) < 1e-6).all()
    assert not np.isnan(long_["t2d"][4:]).any() and (long_["t2d"][4:9] > 0).all() and abs(long_["t2d"][9]) < 1e-6


def test_anchor_against_the_scan_itself():
    """(36, 28) on the fully called copy: every weight is 1 and the closed form is the scan's own T2D / T1D, within
    1e-10 relative wherever those are finite and non-zero."""
    p = PU.genome(N1P, N2P, None, full=True)      # (nothing planted: no under- or over-called SNP)
    assert (p.ref1.astype(int) + p.alt1 == 2 * N1P).all() and (p.ref2.astype(int) + p.alt2 == 2 * N2P).all()
    seen = 0
    for fold in (True, False):
        cfg = _cfg(fold=fold, window=20000)
        with SU.Run(p, cfg) as r:
            recs = r.pl.read()
            st = r.pl.project_scan(36, 28)
        for rec, s in zip(recs, st):
            if rec["flags"] & L.W_EMPTY:
                continue
            for k, f in ((2, "t2d"), (1, "t1d_p1"), (0, "t1d_p2")):
                v = post._v(rec, k)
                assert s["n_dropped"] == 0
                if v is None or not math.isfinite(v) or v == 0.0:
                    continue
                assert abs(float(s[f]) - v) <= 1e-10 * abs(v), (f, float(s[f]), v)
                seen += 1
    assert seen > 100


def test_three_snp_windows_every_workgroup_walks_many():
    """SNP-count windows of 3 SNPs: more than 8 records per resident workgroup, so every workgroup walks several and a
    grid left over from the previous record would show; the all-dropped window is NaN."""
    import torch
    m = (7, 5)
    p = PS.genome(N1P, N2P, m)
    cfg = _cfg(window_mode=L.WINDOW_SNPS, window=3)
    with SU.Run(p, cfg) as r:
        assert r.pl.nrec > 8 * torch.cuda.get_device_properties(0).multi_processor_count
        recs, st = _check(p, r.pl, cfg, m, None, "3-SNP windows")
    at = int(p.chrom_off[-2]) + PS.ALL_DROPPED
    i = int(np.nonzero(recs["begin"] == at)[0][0])
    assert (st["n_used"][i], st["n_dropped"][i], st["n2_fx"][i]) == (0, 3, 0) and all(math.isnan(st[f][i]) for f in FIELDS)
    ok = np.isfinite(st["t2d"]) & (st["t2d"] != 0)
    assert 4 * int(ok.sum()) >= 3 * int((st["n_used"] > 0).sum())


def test_lds_opt_in_grid():
    """(160, 120) from 100 / 75: a 156 kB grid, above the default LDS limit."""
    n1p, n2p, m = 100, 75, (160, 120)
    p = PU.genome(n1p, n2p, m, lengths=BIG)
    cfg = _cfg(n1p, n2p, regions=_whole_chroms(p))
    with SU.Run(p, cfg) as r:
        recs, st = _check(p, r.pl, cfg, m, 0, "161 x 121", exact=False)
        again = r.pl.project_scan(*m, 0)
    assert st.tobytes() == again.tobytes() and st["n_used"].sum() > 2500 and (st["t2d"][1:] > 1.0).all()


def test_grid_beyond_the_lds_is_refused():
    p = PU.genome(127, 127, (254, 254), lengths=[257], full=True)
    cfg = _cfg(127, 127, regions=_whole_chroms(p))
    with SU.Run(p, cfg) as r:
        with pytest.raises(L.Sfs2dError) as ei:
            r.pl.project_scan(254, 254)
        assert ei.value.code == L.E_CAP and "LDS" in str(ei.value)
        assert r.pl.project(254, 254)[1].sum() > 200                        # (sfs2d_plan_project still serves it)


# ------------------------------------------------------------------------------------------- 2. plan kinds

@pytest.mark.parametrize("fused", ["0", "1"], ids=["sliced", "fused"])
def test_tiled_plans(monkeypatch, fused):
    monkeypatch.setenv("SFS2D_FUSED", fused)
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window=20000, prev_extra=True)
    with SU.Run(p, cfg) as r:
        v = r.pl.scan_variant()
        assert v["fused"] == int(fused) and v["cnt"] == 1
        recs, st = _check(p, r.pl, cfg, M, None, f"tiled fused={fused}")
    assert recs[-1]["flags"] & L.W_EXTRA and st["flags"][-1] == L.W_EXTRA and len(recs) > 20
    assert np.isfinite(st["t2d"]).sum() > 15


def test_background_chromosome_long_and_short():
    """SNP-count windows of 65 against one chromosome for every record: the longest (finite) and one of 255 SNPs (+inf
    wherever a window touches a bin it lacks; its own windows finite)."""
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window_mode=L.WINDOW_SNPS, window=65)
    with SU.Run(p, cfg) as r:
        recs, long_ = _check(p, r.pl, cfg, M, 9, "bg_chrom long")
        assert r.pl.project_scan_e_bg == 40
        recs, short = _check(p, r.pl, cfg, M, 4, "bg_chrom short")
        recs, per = _check(p, r.pl, cfg, M, None, "per chromosome")
    assert np.isinf(short["t2d"]).any() and np.isfinite(short["t2d"][recs["chrom"] == 4]).all()
    assert np.isfinite(long_["t2d"][recs["chrom"] == 9]).all() and len(recs) > 200      # (its own windows)
    ok = np.isfinite(per["t2d"]) & (per["t2d"] != 0)
    assert 4 * int(ok.sum()) >= 3 * len(recs)


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
def test_filtered_plan_takes_the_bins(fold):
    """A position filter and variant_type: membership from k_prep's stored bins word (CNT = false)."""
    p = PS.genome(N1P, N2P, M)
    assert p.ann_names[1] == SU.VT
    for kw in ({"window": 20000}, {"window_mode": L.WINDOW_SNPS, "window": 513}):
        cfg = _cfg(fold=fold, **kw, **FILT)
        with SU.Run(p, cfg) as r:
            assert r.pl.scan_variant()["cnt"] == 0
            recs, st = _check(p, r.pl, cfg, M, None, f"filtered {kw}")
        free = PS.twin(p, recs, _cfg(fold=fold, **kw), *M)
        assert 0 < st["n_used"].sum() < free["n_used"].sum() / 2


def test_sliding_plan():
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window=8000, step=2000)
    with SU.Run(p, cfg) as r:
        recs, st = _check(p, r.pl, cfg, M, None, "sliding")
    live = (recs["flags"] & L.W_EMPTY) == 0
    assert live.sum() > 50 and (recs["begin"][live][1:] < recs["end"][live][:-1]).any()      # windows overlap


def test_regions_plan():
    """Overlapping and nested regions, an identical pair, an empty region, a region of more than 2,048 SNPs."""
    from sfs2d.regions import Regions
    p = PS.genome(N1P, N2P, M)
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
            recs, st = _check(p, r.pl, cfg, M, None, f"regions {filt}")
        by = dict(zip(rg.slot_keys(), range(len(recs))))
        assert st[by["empty"]]["flags"] == L.W_EMPTY and recs[by["outer"]]["end"] - recs[by["outer"]]["begin"] > 2048
        assert st[by["nested"]].tobytes() == st[by["nested_again"]].tobytes() and st[by["nested"]]["n_used"] > 0


def test_attached_plans():
    p = PS.genome(N1P, N2P, M)
    for filt in ({}, FILT):
        base_cfg = _cfg(window=2000, **filt)
        cfgs = [_cfg(window=10000, **filt), _cfg(window_mode=L.WINDOW_SNPS, window=65, **filt),
                _cfg(regions=_whole_chroms(p), **filt)]
        with SU.Run(p, base_cfg, run=False) as r:
            att = [r.pl.attach(c) for c in cfgs]
            with pytest.raises(L.Sfs2dError) as ei:      # an attached plan has no records before its base runs
                att[0].project_scan(*M)
            assert ei.value.code == L.E_ARG
            r.pl.run()
            r.pl.check()
            _check(p, r.pl, base_cfg, M, None, "base", twin=not filt)
            for a, c in zip(att, cfgs):
                _check(p, a, c, M, None, f"attached {c.window_mode} {c.window}")


def test_wrapped_device_data():
    import wide_util as WU
    from sfs2d.engine import Engine
    p = PS.genome(N1P, N2P, M)
    for filt, ann in (({}, False), (FILT, True)):
        d, keep = WU.wrapped(Engine.get(0), p, ann=ann)
        try:
            for kw in ({"window": 20000}, {"window": 8000, "step": 4000}):
                cfg = _cfg(**kw, **filt)
                with SU.Run(p, cfg, dev=d) as r:
                    _check(p, r.pl, cfg, M, None, f"wrapped {kw}")
        finally:
            d.close()
        del keep


# ------------------------------------------------------------------------------------------- 3. contract

def test_two_calls_are_byte_equal():
    p = PS.genome(N1P, N2P, M)
    for cfg in (_cfg(window=20000), _cfg(window_mode=L.WINDOW_SNPS, window=7), _cfg(window_mode=L.WINDOW_SNPS, window=513, ann_want=1)):
        with SU.Run(p, cfg) as r:
            a, b = r.pl.project_scan(*M), r.pl.project_scan(*M)
            c = r.pl.project_scan(*M, 9)
            r.pl.project_scan(7, 5)                               # another grid in between
            d, f = r.pl.project_scan(*M, 9), r.pl.project_scan(*M)
            assert a.tobytes() == b.tobytes() == f.tobytes() and c.tobytes() == d.tobytes() and a.tobytes() != c.tobytes()
            assert np.isfinite(a["t2d"]).sum() > 10


@pytest.mark.parametrize("fused", ["0", "1"], ids=["sliced", "fused"])
def test_following_runs_are_untouched(monkeypatch, fused):
    """run, project_scan, run (and once more: both replica parities) leaves the later runs' records and Fst byte-equal
    to a plan that never called it, with diversity, spectra, project and null calls in between, which see what they
    saw -- and sfs2d_plan_project_read still reads the last project call."""
    monkeypatch.setenv("SFS2D_FUSED", fused)
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window=5000, fst=True, prev_extra=True)
    with SU.Run(p, cfg) as ref:
        assert ref.pl.scan_variant()["fused"] == int(fused)
        want = []
        for _ in range(2):
            ref.pl.run()
            ref.pl.check()
            want.append((ref.pl.read().tobytes(), ref.pl.read_fst().tobytes()))
        div, spec = ref.pl.diversity().tobytes(), ref.pl.spectra().tobytes()
        proj = [x.tobytes() for x in ref.pl.project(*M)]
        ref.pl.null_run([(0, 1), (9, 513)], 8, 3)
        null = ref.pl.null_read().tobytes()
    with SU.Run(p, cfg) as r:
        first = None
        for k in range(2):
            s = r.pl.project_scan(*M)
            assert r.pl.spectra().tobytes() == spec and r.pl.diversity().tobytes() == div
            got = r.pl.project(*M)
            assert [x.tobytes() for x in got] == proj
            r.pl.null_run([(0, 1), (9, 513)], 8, 3)
            assert r.pl.null_read().tobytes() == null
            t = r.pl.project_scan(*M)
            assert s.tobytes() == t.tobytes()
            out, uu, dd = np.zeros_like(got[0]), np.zeros_like(got[1]), np.zeros_like(got[2])
            n, w = C.c_int64(), C.c_int64()
            assert r.pl.eng.lib.sfs2d_plan_project_read(r.pl.h, L.ptr(out), L.ptr(uu), L.ptr(dd), len(out), C.byref(n),
                                                        C.byref(w)) == 0 and out.tobytes() == proj[0]
            first = s if first is None else first
            assert s.tobytes() == first.tobytes()      # every run alike
            r.pl.run()
            r.pl.check()
            assert (r.pl.read().tobytes(), r.pl.read_fst().tobytes()) == want[k], k
        _check(p, r.pl, cfg, M, None, "after")


def test_caller_buffer():
    import torch
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window=20000)
    with SU.Run(p, cfg) as r:
        st = r.pl.project_scan(*M)
        e = r.pl.project_scan_e
        buf = torch.full((len(st) * 8 + 8,), 7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        assert r.pl.project_scan(*M, out_dev_ptr=buf.data_ptr()) is None and r.pl.project_scan_e == e
        r.pl.check()                                           # synchronises the engine's stream
        got = buf.cpu().numpy()
        assert (got[len(st) * 8:] == 7).all() and got[:len(st) * 8].tobytes() == st.tobytes()
        # the read call copies from where the last call wrote
        out = np.zeros(len(st), L.PROJSTAT_DTYPE)
        n = C.c_int64()
        assert r.pl.eng.lib.sfs2d_plan_project_scan_read(r.pl.h, L.ptr(out), len(st), C.byref(n)) == 0
        assert n.value == len(st) and out.tobytes() == st.tobytes()


def test_refusals():
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window=20000)
    with SU.Run(p, cfg, run=False) as r:
        lib, h, nrec = r.pl.eng.lib, r.pl.h, r.pl.nrec
        err = lambda: lib.sfs2d_last_error(r.pl.eng.h).decode()
        n, e, eb = C.c_int64(), C.c_int32(), C.c_int32()
        out = np.zeros(nrec, L.PROJSTAT_DTYPE)
        call = lambda m1, m2, bg: lib.sfs2d_plan_project_scan(h, m1, m2, bg, None, C.byref(e), C.byref(eb))
        read = lambda cap: lib.sfs2d_plan_project_scan_read(h, L.ptr(out), cap, C.byref(n))
        assert call(24, 20, -1) == L.E_ARG and "first run" in err()
        assert read(nrec) == L.E_ARG and "before sfs2d_plan_project_scan" in err()         # no call yet
        r.pl.run()
        r.pl.check()
        for m1, m2 in ((1, 20), (37, 20), (24, 1), (24, 29), (0, 0), (-3, 20)):
            assert call(m1, m2, -1) == L.E_ARG and "outside [2, 36] x [2, 28]" in err(), (m1, m2)
        for bg in (-2, p.nchrom, 1 << 20):
            assert call(24, 20, bg) == L.E_ARG and "bg_chrom" in err(), bg
        assert read(nrec) == L.E_ARG                                                       # still none
        assert call(24, 20, p.nchrom - 1) == 0 and (e.value, eb.value) == (40, 40)
        assert lib.sfs2d_plan_project_scan(h, 24, 20, -1, None, None, None) == 0           # the exponents are optional
        assert read(nrec - 1) == L.E_CAP and n.value == nrec
        assert read(nrec) == 0 and np.isfinite(out["t2d"]).sum() > 15
    # a plan with a supplied background
    cfg = _cfg(window=20000, bg_mode=L.BG_SUPPLIED)
    bg = (np.ones((2 * N1P + 1) * (2 * N2P + 1)), np.ones(N1P + 1), np.ones(N2P + 1))
    with SU.Run(p, cfg, bg=bg) as r:
        with pytest.raises(L.Sfs2dError) as ei:
            r.pl.project_scan(*M)
        assert ei.value.code == L.E_ARG and "supplied background" in str(ei.value)


# ------------------------------------------------------------------------------------------- 4. class and CLI

def test_class_projected_scan():
    import twoDSFS_class as T
    from sfs2d.regions import Regions
    p = PS.genome(N1P, N2P, M)
    names = p.chrom_names
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=N1P, pop2_size=N2P)
    for kw, ckw, kind in (({"window_size": 20000}, {"window": 20000}, "bp"),
                          ({"window_size": 8000, "step_size": 2000}, {"window": 8000, "step": 2000}, "bp"),
                          ({"snp_window_size": 257}, {"window_mode": L.WINDOW_SNPS, "window": 257}, "snps")):
        for bgname in (None, names[9]):
            cfg = _cfg(**ckw)
            with SU.Run(p, cfg) as r:
                recs = r.pl.read()
                st = r.pl.project_scan(*M, None if bgname is None else 9)
            want = SP.project_scan_rows(recs, st, post.record_labels(recs, p, kind, ckw["window"], ckw.get("step")))
            got = obj.projected_scan(p, M, background_chromosome=bgname, **kw)
            assert got == want and len(got) > 20 and list(got) == list(want)
            assert sum(v["T2D_proj"] is not None for v in got.values()) > 15
    c9 = names[9]
    items = [(c9, 10000, 200000, "outer"), (names[8], 1, 1 << 31, "chrom8"), (c9, 1 << 30, 1 << 31, "empty"),
             (c9, 50000, 60000, "nested")]
    got = obj.projected_scan(p, M, regions=items)
    assert list(got) == ["outer", "chrom8", "empty", "nested"]
    assert got["empty"]["snp_count"] == 0 and got["empty"]["T2D_proj"] is None and got["empty"]["n_used"] == 0
    rg = Regions(names, items)
    cfg = _cfg(regions=rg)
    with SU.Run(p, cfg) as r:
        recs, st = r.pl.read(), r.pl.project_scan(*M)
    order = rg.slot.tolist()
    assert got == SP.project_scan_rows(recs[order], st[order], list(rg.keys())) and got["outer"]["T2D_proj"] > 0
    c8 = got["chrom8"]      # a chromosome against itself
    _, wu, wd = PU.twin(p, None, PU.Cfg(N1P, N2P), *M, rec=[-9])
    assert abs(c8["T2D_proj"]) < 1e-6 and (c8["n_used"], c8["n_dropped"]) == (int(wu[0]), int(wd[0])) and wu[0] > 1000


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_cli_outputs(tmp_path, capsys):
    import csv
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
            "--snp-window", "100", "--regions", str(bed)]
    plain = cli.main(base + ["--out-prefix", str(tmp_path / "p")])
    capsys.readouterr()
    outs = cli.main(base + ["--project-scan", "16,14", "--out-prefix", str(tmp_path / "s")])
    errtext = capsys.readouterr().err
    names = lambda paths, pre: sorted(os.path.basename(x)[len(pre):] for x in paths)
    assert not any("_projscan" in n for n in names(plain, "p"))
    assert names(outs, "s") == sorted(names(plain, "p") + [n[:-4] + "_projscan16x14.csv" for n in names(plain, "p")])
    for a in plain:      # every old file is what it was
        assert _read(a) == _read(str(tmp_path / ("s" + os.path.basename(a)[1:])))
    assert errtext.count("SNPs dropped (") == 3 and "projected_scan (16, 14)" in errtext
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=11, pop2_size=11)
    for stem, kw in (("s_500kb", {"window_size": 500000}), ("s_100snps", {"snp_window_size": 100}),
                     ("s_regions", {"regions": str(bed)})):
        want = obj.projected_scan(p, (16, 14), **kw)
        with open(tmp_path / (stem + "_projscan16x14.csv"), newline="") as fh:
            rows = list(csv.DictReader(fh))
        head = (["name"] if "regions" in kw else []) + ["chromosome", "window_start", "window_end"]
        assert list(rows[0]) == head + SP.PROJSCAN_COLUMNS and len(rows) == len(want)
        for row, (lb, w) in zip(rows, want.items()):
            if "regions" in kw:
                assert row["name"] == lb
            else:
                assert f"{row['chromosome']} {row['window_start']}-{row['window_end']}" == lb
            for k in SP.PROJSCAN_COLUMNS:
                assert row[k] == ("" if w[k] is None else str(w[k])), (stem, lb, k)
    assert any(w["T2D_proj"] is not None and w["T2D_proj"] > 0 for w in want.values()) and want["empty"]["T2D_proj"] is None
