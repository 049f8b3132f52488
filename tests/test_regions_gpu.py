"""Regions plans (sfs2d_plan_create_regions / sfs2d_plan_attach_regions) against the oracle, region by region.

The genome, the region list and the reference are regions_util's (its docstring lists what the list holds): the
expected SNP range of every slot is built there from the definition with np.searchsorted, and O.window_records /
O.window_fst of the same O.Cfg give each non-empty region's values: integers exact, T by golden_util.close with
None exactly where the oracle has None, Fst within 1e-12 + 1e-10 |x|.  Slot i of a plan is region i of the list
sorted stably by chromosome (sfs2d.regions.Regions); an empty region is an SFS2D_W_EMPTY record with (0, 0).
Every plan is run twice (run, then run_many(2)) and the second table must equal the first."""
import csv
import ctypes as C
import os

import numpy as np
import pytest

import golden_util as gu
import regions_util as RU
from oracle import sfs_oracle as O

pytestmark = pytest.mark.gpu

W, S = 6400, 1600
VT = RU.VT


@pytest.fixture(autouse=True)
def _small_tiles(monkeypatch):
    monkeypatch.setenv("SFS2D_TILE", "4096")
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG"):
        monkeypatch.delenv(k, raising=False)


def _cfg(p, n1p, n2p, rg=None, vt=None, fold=True, start=None, **kw):
    from sfs2d import _lib as L
    from sfs2d.engine import ScanConfig
    return ScanConfig(n1p=n1p, n2p=n2p, fold=fold, window_mode=L.WINDOW_BP, start_position=start,
                      ann_want=-1 if vt is None else p.ann_names.index(vt), regions=rg, **kw)


def _run_on(dev, cfg, bg=None, kernel=None, bytes_equal=True):
    """run, then run_many(2), of one plan on resident data: (records, Fst, scan_variant, seg_kind); the replay's
    table is the first run's, byte for byte (bytes_equal False: integers and Fst byte for byte, T by close)."""
    pl = dev.eng.plan(dev, cfg)
    try:
        if kernel is not None:
            assert pl.scan_kernel() == kernel, pl.scan_kernel()
        if bg is not None:
            pl.set_background(*bg)
        pl.run()
        pl.check()
        r0, f0 = pl.read(), pl.read_fst() if cfg.fst else None
        pl.run_many(2)
        pl.check()
        r1, f1 = pl.read(), pl.read_fst() if cfg.fst else None
        var, seg = pl.scan_variant(), pl.seg_kind()
    finally:
        pl.close()
    RU.same_ints(r0, r1, f0, f1)
    if bytes_equal:
        assert r0.tobytes() == r1.tobytes()
    else:
        RU.same_t(r0, r1)
    return r0, f0, var, seg


def _run(p, cfg, **kw):
    from sfs2d.engine import Engine
    dev = Engine.get(0).upload(p)
    try:
        return _run_on(dev, cfg, **kw)
    finally:
        dev.close()


KERNELS = {"w_fused": (18, 14, {"SFS2D_FUSED": "1"}, "k_scan_w"), "w_sliced": (18, 14, {"SFS2D_FUSED": "0"}, "k_scan_w"),
           "gw": (50, 50, {"SFS2D_GW": "1"}, "k_scan_gw"), "g": (50, 50, {"SFS2D_GW": "0"}, "k_scan_g")}


# ------------------------------------------------------------------------------------------- scan kernels

@pytest.mark.parametrize("path", list(KERNELS))
def test_scan_kernels(monkeypatch, path):
    """Per-chromosome backgrounds, folded, with Fst (summed by k_scan_w's scan; k_fst_win on the large grids) on
    every scan kernel; without Fst the integers are the same."""
    n1p, n2p, env, kernel = KERNELS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = RU.genome(n1p, n2p)
    rg = RU.regions(p)
    ref = RU.reference(n1p, n2p)
    recs, fst, var, seg = _run(p, _cfg(p, n1p, n2p, rg, fst=True), kernel=kernel)
    assert seg == "regions"
    assert var["p16"] == 1   # no region of 65,536 SNPs, counted from the host copy of the positions
    assert (var["fst"] >= 2) == (kernel == "k_scan_w")   # Fst by the scan / by k_fst_win before it
    RU.check(recs, fst, ref)
    from sfs2d.regions import region_ranges
    b, e = region_ranges(p, rg)
    assert [(x[2], x[3]) for x in ref[0]] == list(zip(b.tolist(), e.tolist()))
    nof, _, _, _ = _run(p, _cfg(p, n1p, n2p, rg), kernel=kernel)
    RU.check(nof, None, ref)
    RU.same_ints(recs, nof)


@pytest.mark.parametrize("case", ["filtered_fused", "filtered_sliced", "supplied", "supplied_fst", "fst_win_counts",
                                  "unfolded"])
def test_plan_flavours(monkeypatch, case):
    """A variant_type + start_position filter on the bins pipeline (Fst by k_fst_win from the bins words); a
    supplied background (a counts plan launches k_slots_regions and the scan alone), with and without Fst; a
    counts plan whose Fst is k_fst_win's (SFS2D_FST_SCAN=0); unfolded spectra."""
    from sfs2d import _lib as L
    n1p, n2p = 18, 14
    p = RU.genome(n1p, n2p)
    rg = RU.regions(p)
    kw, okw, bg, want_fst = {}, {}, None, None
    if case.startswith("supplied"):
        okw = dict(bg_chrom=4)
        kw = dict(bg_mode=L.BG_SUPPLIED, fst=case == "supplied_fst")
        bg = O.chrom_backgrounds(p, O.Cfg(n1p, n2p))[4]
    elif case == "unfolded":
        okw = dict(fold=False)
        kw = dict(fold=False, fst=True)
    elif case.startswith("filtered"):
        start = int(p.pos[int(p.chrom_off[4]) + 4096 + 1])   # the second SNP of a lane's four, after a tile edge
        okw = dict(vt=VT, start=start)
        kw = dict(vt=VT, start=start, fst=True)
        monkeypatch.setenv("SFS2D_FUSED", "0" if case == "filtered_sliced" else "1")
        want_fst = 0
    else:
        monkeypatch.setenv("SFS2D_FST_SCAN", "0")
        kw = dict(fst=True)
        want_fst = 0
    recs, fst, var, seg = _run(p, _cfg(p, n1p, n2p, rg, **kw), bg=bg, kernel="k_scan_w")
    assert seg == "regions"
    if want_fst is not None:
        assert var["fst"] == want_fst, var   # never k_prep's fixed-point sums (1): k_fst_win wrote Fst
    RU.check(recs, fst, RU.reference(n1p, n2p, **okw))


# ------------------------------------------------------------------------------------------- equivalences

def _tile_regions(p, w, s):
    """The regions (j s + 1, j s + w) of every slot of the sliding geometry (w, s); slot 0 starts at 0, as the
    sliding plan's slot 0 holds a SNP at position 0."""
    from sfs2d.regions import Regions
    items = []
    for c in range(p.nchrom):
        lo, hi = int(p.chrom_off[c]), int(p.chrom_off[c + 1])
        if lo == hi:
            continue
        last = int(p.pos[hi - 1])
        for j in range((last - 1) // s + 1 if last else 1):
            items.append((p.chrom_names[c], j * s + 1 if j else 0, j * s + w))
    return Regions(p.chrom_names, items)


@pytest.mark.parametrize("path", ["w_fused", "w_sliced"])
def test_equals_the_sliding_plan(monkeypatch, path):
    """The regions of every sliding slot give the sliding plan's records and Fst byte for byte (the same scan
    kernel over the same slot table)."""
    n1p, n2p, env, kernel = KERNELS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = RU.genome(n1p, n2p)
    rg = _tile_regions(p, W, S)
    slide, sf, _, seg = _run(p, _cfg(p, n1p, n2p, window=W, step=S, fst=True), kernel=kernel)
    assert seg == "slide" and (slide["flags"] & 0x80000000).any()
    recs, fst, _, seg = _run(p, _cfg(p, n1p, n2p, rg, fst=True), kernel=kernel)
    assert seg == "regions" and len(recs) == len(slide)
    assert recs.tobytes() == slide.tobytes()
    assert fst.tobytes() == sf.tobytes()


def test_equals_the_tiled_plan():
    """The tiles of an ordinary 20 kb plan as regions: equal integers, T and Fst within tolerance."""
    n1p, n2p = 18, 14
    p = RU.genome(n1p, n2p)
    rg = _tile_regions(p, 20000, 20000)
    plain, pf, _, _ = _run(p, _cfg(p, n1p, n2p, window=20000, fst=True), kernel="k_scan_w")
    recs, fst, _, _ = _run(p, _cfg(p, n1p, n2p, rg, fst=True), kernel="k_scan_w")
    assert len(recs) == len(plain) == len(rg)
    RU.same_ints(recs, plain)
    RU.same_t(recs, plain)
    for g, f in zip(fst, pf):
        assert (np.isnan(g) and np.isnan(f)) or abs(g - f) <= 1e-12 + 1e-10 * abs(f), (g, f)


# ------------------------------------------------------------------------------------------- attached plans

@pytest.mark.parametrize("path", ["w_fused", "w_sliced", "gw"])
def test_attached_regions_plans(monkeypatch, path):
    """A regions plan (Fst) attached to an ordinary base (window S) and to a sliding base (2 S by S, Fst): the
    standalone plan's table byte for byte (large grid: integers and Fst byte for byte, T by close), twice; the
    base's own records are what the base gives alone."""
    from sfs2d.engine import Engine
    n1p, n2p, env, kernel = KERNELS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = RU.genome(n1p, n2p)
    rg = RU.regions(p)
    ref = RU.reference(n1p, n2p)
    exact = kernel == "k_scan_w"
    dev = Engine.get(0).upload(p)
    try:
        alone, alone_f, _, _ = _run_on(dev, _cfg(p, n1p, n2p, rg, fst=True), kernel=kernel, bytes_equal=exact)
        for base_cfg in (_cfg(p, n1p, n2p, window=S), _cfg(p, n1p, n2p, window=2 * S, step=S, fst=True)):
            want, want_f, _, _ = _run_on(dev, base_cfg, kernel=kernel, bytes_equal=exact)
            base = dev.eng.plan(dev, base_cfg)
            att = base.attach(_cfg(p, n1p, n2p, rg, fst=True))
            assert att.scan_kernel() == kernel and att.seg_kind() == "regions"
            for _ in range(2):
                base.run()
                base.check()
                att.check()
                recs, fst = att.read(), att.read_fst()
                RU.same_ints(recs, alone, fst, alone_f)
                if exact:
                    assert recs.tobytes() == alone.tobytes()
                else:
                    RU.same_t(recs, alone)
                RU.check(recs, fst, ref)
                mine = base.read()
                RU.same_ints(mine, want, base.read_fst() if base_cfg.fst else None, want_f)
                if exact:
                    assert mine.tobytes() == want.tobytes()
                else:
                    RU.same_t(mine, want)
            base.close()
        # an ordinary plan attached to a regions base: possible, and the oracle's
        base = dev.eng.plan(dev, _cfg(p, n1p, n2p, rg, fst=True))
        att = base.attach(_cfg(p, n1p, n2p, window=2 * S, step=S, fst=True))
        base.run()
        base.check()
        att.check()
        RU.check(base.read(), base.read_fst(), ref)
        want, want_f, _, _ = _run_on(dev, _cfg(p, n1p, n2p, window=2 * S, step=S, fst=True), bytes_equal=exact)
        RU.same_ints(att.read(), want, att.read_fst(), want_f)
        base.close()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------- wide bins

_WIDE = {}


def _wide_genome():
    """One chromosome of 70,000 SNPs (positions 2, 4, ...) and the region that covers it."""
    if not _WIDE:
        from sfs2d.pack import PackedSNPs, pack_counts
        from sfs2d.regions import Regions
        from sfs2d.synth import synth_chrom
        rng = np.random.Generator(np.random.PCG64(70))
        n = 70000
        _, r1, a1, r2, a2 = synth_chrom(rng, n, 18, 14)
        p = PackedSNPs(pack_counts(r1, a1, r2, a2), (2 * np.arange(1, n + 1)).astype(np.uint32),
                       np.array([0, n], np.int64), ["chrW"], np.zeros(n, np.uint16), ["x"], "p1", "p2")
        rg = Regions(p.chrom_names, [("chrW", 1, 200000, "all"), ("chrW", 3, 20, "small")])
        slots = RU.slots_of(p, rg)
        assert slots[0][2:] == (0, n) and slots[1][3] - slots[1][2] == 9
        ref = RU.oracle_of(p, slots, O.Cfg(18, 14))
        RU.no_cancelled_t(o[t] for o in ref[1] for t in ("T2D", "T1D_p1", "T1D_p2"))
        _WIDE["v"] = (p, rg, ref)
    return _WIDE["v"]


def test_wide_bins_uploaded():
    """A region of 70,000 SNPs on uploaded data: the exact count from the host copy of the positions selects the
    32-bit-bin instantiation; without it the same data take 16-bit bins."""
    p, rg, ref = _wide_genome()
    recs, fst, var, _ = _run(p, _cfg(p, 18, 14, rg, fst=True), kernel="k_scan_w")
    assert var["p16"] == 0, var
    RU.check(recs, fst, ref)
    from sfs2d.regions import Regions
    small = Regions(p.chrom_names, [("chrW", 3, 20, "small"), ("chrW", 1, 131070, "most")])   # 65,535 SNPs
    _, _, var, _ = _run(p, _cfg(p, 18, 14, small, fst=True), kernel="k_scan_w")
    assert var["p16"] == 1, var


def test_wide_bins_wrapped():
    """Wrapped device arrays have no host copy of the positions: 32-bit bins whatever the regions hold."""
    import wide_util as WU
    from sfs2d.engine import Engine
    p = RU.genome(18, 14)
    rg = RU.regions(p)
    dev, keep = WU.wrapped(Engine.get(0), p)
    try:
        recs, fst, var, seg = _run_on(dev, _cfg(p, 18, 14, rg, fst=True), kernel="k_scan_w")
    finally:
        dev.close()
    del keep
    assert var["p16"] == 0 and seg == "regions", (var, seg)
    RU.check(recs, fst, RU.reference(18, 14))


# ------------------------------------------------------------------------------------------- diversity, null

@pytest.mark.parametrize("path", ["w_sliced", "gw"])
def test_diversity_and_null(monkeypatch, path):
    """Plan.diversity after a regions run = sfs2d.diversity.window_sums over the reference ranges (integers exact,
    the fp64 sums within 1e-12 relative); a null run with tasks from two regions' SNP counts = null.resample
    evaluated by the oracle; the run after both is the run before, byte for byte."""
    from sfs2d import _lib as L
    from sfs2d import diversity as DV
    from sfs2d.engine import Engine
    import null_util as NU
    n1p, n2p, env, kernel = KERNELS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = RU.genome(n1p, n2p)
    rg = RU.regions(p)
    slots = RU.reference(n1p, n2p)[0]
    cfg = _cfg(p, n1p, n2p, rg, fst=True)
    dev = Engine.get(0).upload(p)
    try:
        pl = dev.eng.plan(dev, cfg)
        pl.run()
        pl.check()
        r0, f0 = pl.read(), pl.read_fst()
        div = pl.diversity()
        want = DV.window_sums(p, [x[2] for x in slots], [x[3] for x in slots], cfg)
        want["flags"] = [L.W_EMPTY if x[2] == x[3] else 0 for x in slots]
        for f in ("ar1_full", "ar2_full", "s1", "s2", "s1_full", "s2_full", "flags", "reserved"):
            assert np.array_equal(div[f], want[f]), f
        for f in ("pi1", "pi2", "dxy", "thw1", "thw2"):
            for i, (g, w) in enumerate(zip(div[f].tolist(), want[f].tolist())):
                assert (g == 0.0) if w == 0.0 else abs(g - w) <= 1e-12 * abs(w), (f, i, g, w)
        assert max(int(d["s1"]) for d in div) > 512
        # two size classes from the list: the SNP counts of "nested" and "from_snp", each on its own chromosome
        by_key = dict(zip(rg.slot_keys(), slots))
        tasks = [(by_key[k][0], by_key[k][3] - by_key[k][2]) for k in ("nested", "from_snp")]
        assert tasks[0][0] == 4 and tasks[1][0] == 2 and all(m > 64 for _, m in tasks)
        R, seed = 19, 11
        pl.null_run(tasks, R, seed)
        got = pl.null_read()
        ocfg = O.Cfg(n1p, n2p)
        bgs = O.chrom_backgrounds(p, ocfg)
        twin, _, _ = NU.null_twin(p, tasks, R, seed, ocfg, lambda c: bgs[c])
        assert len(got) == len(twin) == 2 * R
        for f in RU.INTS:
            assert np.array_equal(got[f], twin[f]), f
        for f in ("t2d", "t1d_p1", "t1d_p2"):
            for g, w in zip(got[f].tolist(), twin[f].tolist()):
                assert gu.close(g, w, scale=1e-2), (f, g, w)   # (test_null_gpu's floor for resampled windows)
        pl.run()
        pl.check()
        r1, f1 = pl.read(), pl.read_fst()
        RU.same_ints(r0, r1, f0, f1)
        if kernel == "k_scan_w":
            assert r0.tobytes() == r1.tobytes()
        else:
            RU.same_t(r0, r1)
        pl.close()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------- streams, graph

def test_streams_and_graph():
    """Two regions plans round-robin on two streams (sfs2d_plan_run_streams), then captured and replayed
    (sfs2d_graph_*): each writes what the same plan writes run alone."""
    import torch
    from sfs2d import _lib as L
    from sfs2d.engine import Engine, Plan
    p = RU.genome(18, 14)
    cfg = _cfg(p, 18, 14, RU.regions(p), fst=True)
    want, want_f, _, _ = _run(p, cfg, kernel="k_scan_w")
    RU.check(want, want_f, RU.reference(18, 14))
    eng = Engine.get(0)
    dev = eng.upload(p)
    plans = [eng.plan(dev, cfg) for _ in range(2)]
    streams = [torch.cuda.Stream(device=0).cuda_stream for _ in range(2)]
    outs = [torch.zeros((plans[0].nrec, 64), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    optrs = [o.data_ptr() for o in outs]

    def check_all():
        torch.cuda.synchronize()
        for k, q in enumerate(plans):
            q.check()
            got = np.frombuffer(outs[k].cpu().numpy().tobytes(), dtype=L.WINDOW_DTYPE)
            assert got.tobytes() == want.tobytes()
            assert q.read_fst().tobytes() == want_f.tobytes()

    Plan.run_streams(plans, streams, 5, optrs)
    check_all()
    g = Plan.graph(plans, streams, 4, optrs)
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    g.launch(1)
    check_all()
    g.close()
    for q in plans:
        q.close()
    dev.close()


def test_live_timing():
    """Live timing (sfs2d_plan_set_timing) and sfs2d_plan_time on regions plans: with per-chromosome backgrounds the
    first stage is k_prep, with a supplied background (no k_prep) it is k_slots_regions itself, which then carries
    the stage's events; the timed runs write the untimed table."""
    from sfs2d import _lib as L
    from sfs2d.engine import Engine
    p = RU.genome(18, 14)
    rg = RU.regions(p)
    bg = O.chrom_backgrounds(p, O.Cfg(18, 14))[4]
    dev = Engine.get(0).upload(p)
    try:
        for kw, b in ((dict(fst=True), None), (dict(bg_mode=L.BG_SUPPLIED), bg)):
            cfg = _cfg(p, 18, 14, rg, **kw)
            want, _, _, _ = _run_on(dev, cfg, bg=b)
            pl = dev.eng.plan(dev, cfg)
            if b is not None:
                pl.set_background(*b)
            pl.set_timing(2)
            pl.run_many(2)
            pl.check()
            n, (k1, k2, k3) = pl.timing_read()
            assert n == 2 and k1 > 0.0 and k3 > 0.0, (n, k1, k2, k3)
            assert pl.read().tobytes() == want.tobytes()
            ms = pl.time(2)
            assert all(x > 0.0 for x in (ms[0], ms[1], ms[3])), ms
            assert pl.read().tobytes() == want.tobytes()
            pl.close()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------- refusals

def test_refusals():
    """Every refusal of the two entry points, with its reason; an ordinary plan on the same ctx afterwards still
    matches the oracle."""
    from sfs2d import _lib as L
    from sfs2d.engine import Engine
    p = RU.genome(18, 14)
    eng = Engine.get(0)
    dev = eng.upload(p)
    base = eng.plan(dev, _cfg(p, 18, 14, window=S))
    ok = _cfg(p, 18, 14).params()
    snp = _cfg(p, 18, 14).params()
    snp.window_mode, snp.window = L.WINDOW_SNPS, 64
    q9 = _cfg(p, 18, 14, prev_extra=True).params()
    i32 = lambda v: np.asarray(v, np.int32)
    u32 = lambda v: np.asarray(v, np.uint32)
    good = (i32([0, 2, 4]), u32([1, 5, 0]), u32([100, 5, 0xFFFFFFFF]))
    cases = [(ok, (None, good[1], good[2]), 3, "null array"), (ok, (good[0], None, good[2]), 3, "null array"),
             (ok, (good[0], good[1], None), 3, "null array"), (ok, good, 0, "at least one"), (ok, good, -1, "at least one"),
             (ok, good, 1 << 31, "fewer than 2^31"),
             (ok, (i32([0, 5, 5]), good[1], good[2]), 3, "chrom out of range at region 1"),
             (ok, (i32([-1, 0, 0]), good[1], good[2]), 3, "chrom out of range at region 0"),
             (ok, (i32([0, 4, 2]), good[1], good[2]), 3, "chrom decreases at region 2"),
             (ok, (good[0], u32([1, 6, 0]), good[2]), 3, "first > last at region 1"),
             (q9, good, 3, "SFS2D_F_PREV_EXTRA"), (snp, good, 3, "SNP-count")]
    for prm, (c, f, l), n, why in cases:
        for attach in (False, True):
            h = C.c_void_p()
            args = (C.byref(prm), L.ptr(c), L.ptr(f), L.ptr(l), n, C.byref(h))
            rc = eng.lib.sfs2d_plan_attach_regions(base.h, *args) if attach else \
                eng.lib.sfs2d_plan_create_regions(eng.h, dev.h, *args)
            msg = eng.lib.sfs2d_last_error(eng.h).decode()
            assert rc == L.E_ARG and why in msg and not h.value, (why, attach, rc, msg)
    h = C.c_void_p()   # the same arrays are a plan when nothing is wrong with them
    assert eng.lib.sfs2d_plan_create_regions(eng.h, dev.h, C.byref(ok), *[L.ptr(a) for a in good], 3, C.byref(h)) == 0
    assert eng.lib.sfs2d_plan_num_records(h) == 3
    eng.lib.sfs2d_plan_destroy(h)
    base.close()
    dev.close()
    rg = RU.regions(p)
    recs, fst, _, _ = _run(p, _cfg(p, 18, 14, rg, fst=True), kernel="k_scan_w")
    RU.check(recs, fst, RU.reference(18, 14))


# ------------------------------------------------------------------------------------------- class, CLI

def test_class_methods():
    """region_scan (per-chromosome backgrounds and a named background chromosome), regions= on multi_scan,
    multi_sliding_scan and scan_pvalues: rows built from the oracle's records by the clean rule, one per region in
    the caller's order; the tiled results beside them are what the same call gives without regions."""
    import twoDSFS_class as T
    from sfs2d import diversity as DV
    from sfs2d import null as N
    p = RU.genome(18, 14)
    rg = RU.regions(p)
    its = RU.items(p)
    obj = T.LikelihoodInference_jointSFS(None, None, pop1=p.pop1, pop2=p.pop2, pop1_size=18, pop2_size=14)
    want = RU.clean_rows(rg, RU.reference(18, 14), True)
    assert list(want) == [it[3] for it in its]
    RU.compare_rows(obj.region_scan(p, its, fst=True), want)
    RU.compare_rows(obj.region_scan(p, rg, background_chromosome="chr0004"),
                    RU.clean_rows(rg, RU.reference(18, 14, bg_chrom=4), False))
    with pytest.raises(ValueError, match="Background chromosome nope not found in the data."):
        obj.region_scan(p, rg, background_chromosome="nope")
    # diversity columns: per site of the region's own length; an empty region: None
    rows = obj.region_scan(p, rg, diversity=True)
    slots = RU.reference(18, 14)[0]
    sums = DV.window_sums(p, [x[2] for x in slots], [x[3] for x in slots], _cfg(p, 18, 14))
    for key, s in zip(rg.keys(), rg.slot.tolist()):
        row, (c, j, b, e) = rows[key], slots[s]
        if b == e:
            assert all(row[k] is None for k in DV.KEYS) and row["snp_count"] == 0, key
            continue
        span = int(rg.last[s]) - int(rg.first[s]) + 1
        assert row["S_pop1"] == int(sums["s1"][s]) and row["S_full_pop2"] == int(sums["s2_full"][s]), key
        for k, f in (("pi_pop1", "pi1"), ("pi_pop2", "pi2"), ("dxy", "dxy"), ("theta_w_pop1", "thw1")):
            w = float(sums[f][s]) / span
            assert abs(row[k] - w) <= 1e-12 * abs(w), (key, k, row[k], w)
    # beside a tiled and a sliding scan, from one pass
    # (500-SNP windows: combined_scan's driver raises on this genome's first, monomorphic window as the reference
    # does, quirk Q6; test_cli_regions has the fixed-bp tiles beside the regions)
    multi = obj.multi_scan(p, snp_window_sizes=[500], fst=True, regions=its)
    plain = obj.multi_scan(p, snp_window_sizes=[500], fst=True)
    assert list(multi) == ["500snps", "regions"] and multi["500snps"] == plain["500snps"] and len(plain["500snps"]) > 10
    RU.compare_rows(multi["regions"], want)
    slide = obj.multi_sliding_scan(p, [W], S, fst=True, regions=rg)
    assert list(slide) == [W, "regions"] and list(slide[W]) == list(obj.multi_sliding_scan(p, [W], S, fst=True)[W])
    RU.compare_rows(slide["regions"], want)
    RU.compare_rows(obj.multi_scan(p, regions=rg, fst=True)["regions"], want)
    # p-values: a region's pool is its chromosome, its m its SNP count (sizes="exact": its own class)
    R, seed = 19, 3
    res = obj.scan_pvalues(p, snp_window_sizes=[500], regions=rg, replicates=R, seed=seed, sizes="exact", fst=True)
    assert list(res) == ["500snps", "regions"]
    pv_rows = res["regions"]
    RU.compare_rows({k: {a: b for a, b in r.items() if not a.startswith("p_")} for k, r in pv_rows.items()}, want)
    ocfg = O.Cfg(18, 14)
    bgs = O.chrom_backgrounds(p, ocfg)
    import null_util as NU
    live = [(key, slots[s]) for key, s in zip(rg.keys(), rg.slot.tolist()) if slots[s][2] < slots[s][3]]
    tasks = sorted(set((x[0], x[3] - x[2]) for _, x in live))
    twin, _, _ = NU.null_twin(p, tasks, R, seed, ocfg, lambda c: bgs[c])
    obs = NU.oracle_records(p, [x for _, x in live], ocfg, lambda c: bgs[c])
    classes = np.array([x[3] - x[2] for _, x in live], np.int64)
    pv = N.pvalues(obs, twin, classes)   # the p-value rule over the host twin of the draws, evaluated by the oracle
    for i, (key, x) in enumerate(live):
        for k in N.P_KEYS:
            g, w = pv_rows[key][k], pv[k][i]
            assert (g is None) if np.isnan(w) else (g is not None and abs(g - w) <= 1e-12), (key, k, g, w)
    for key, s in zip(rg.keys(), rg.slot.tolist()):
        if slots[s][2] == slots[s][3]:
            assert all(pv_rows[key][k] is None for k in N.P_KEYS), key   # an empty region: None
    bgp = obj.scan_pvalues(p, regions=rg, background_chromosome="chr0004", replicates=R, seed=seed)
    assert list(bgp) == ["regions"]
    RU.compare_rows({k: {a: b for a, b in r.items() if not a.startswith("p_")} for k, r in bgp["regions"].items()},
                    RU.clean_rows(rg, RU.reference(18, 14, bg_chrom=4), False))
    assert all(all(k in r for k in N.P_KEYS) for r in bgp["regions"].values())


def _vcf():
    return os.path.join(gu.GOLD, "vcf_test.vcf.gz"), os.path.join(gu.GOLD, "popmap_ref.txt")


def _read_csv(path):
    with open(path, newline="") as fh:
        return list(csv.DictReader(fh))


def test_cli_regions(tmp_path):
    """--regions alone and beside --window, with --fst --diversity --null-replicates 19: <prefix>_regions.csv has a
    leading name column, then the usual columns in the usual order, one row per BED line in the file's order, the
    statistics those of rows built from the oracle; the tiled file beside it is the one the same command writes
    without --regions."""
    import twoDSFS_class as T
    from sfs2d import cli
    from sfs2d import diversity as DV
    from sfs2d.regions import Regions
    from sfs2d.vcf import read_vcf
    vcf, pm = _vcf()
    p = read_vcf(vcf, pm).to_packed("uv", "bv")
    c0 = p.chrom_names[0]
    lo, hi = int(p.chrom_off[0]), int(p.chrom_off[1])
    pos = p.pos[lo:hi].astype(np.int64)
    assert hi - lo > 40
    last = int(pos[-1])
    bed = tmp_path / "genes.bed"
    lines = [f"# genes\n", f"{c0}\t{int(pos[10]) - 1}\t{int(pos[30])}\tgeneA\n", f"{c0}\t{last + 10}\t{last + 20}\tempty\n",
             f"{c0}\t0\t{last}\n", f"{p.chrom_names[-1]}\t0\t4000000000\tlastchrom\n", f"{c0}\t{int(pos[5]) - 1}\t{int(pos[5])}\n"]
    bed.write_text("".join(lines))
    rg = Regions.from_bed(p, str(bed))
    assert rg.keys() == ["geneA", "empty", f"{c0} 1-{last}", "lastchrom", f"{c0} {int(pos[5])}-{int(pos[5])}"]
    slots = RU.slots_of(p, rg)
    want = RU.clean_rows(rg, RU.oracle_of(p, slots, O.Cfg(18, 14)), True)
    flags = ["--fst", "--diversity", "--null-replicates", "19"]
    outs = cli.main([vcf, pm, "--regions", str(bed), "--out-prefix", str(tmp_path / "A")] + flags)
    assert [os.path.basename(o) for o in outs] == ["A_regions.csv"]
    # (500 kb tiles: at 20 kb combined_scan's driver raises on this LD-pruned data as the reference does, quirk Q6,
    # test_cli.test_cli_end_to_end)
    both = cli.main([vcf, pm, "--regions", str(bed), "--window", "500000", "--out-prefix", str(tmp_path / "B")] + flags)
    assert [os.path.basename(o) for o in both] == ["B_500kb.csv", "B_regions.csv"]
    only = cli.main([vcf, pm, "--window", "500000", "--out-prefix", str(tmp_path / "C")] + flags)
    assert open(both[0], "rb").read() == open(only[0], "rb").read()
    txt = lambda v: "" if v is None else str(v)
    for path in (outs[0], both[1]):
        rows = _read_csv(path)
        assert list(rows[0]) == ["name"] + T.col_names + ["FST"] + DV.KEYS + cli.P_COLS
        assert [r["name"] for r in rows] == list(want)
        for r, (key, o), s in zip(rows, want.items(), rg.slot.tolist()):
            assert (r["window_start"], r["window_end"]) == (str(int(rg.first[s])), str(int(rg.last[s]))), key
            assert r["snp_count"] == str(o["snp_count"]), key
            for col, k in (("T2D", "T2D"), ("T1D_p1", "T1D_pop1"), ("T1D_p2", "T1D_pop2"), ("T2D_diff", "T2D_diff"), ("FST", "FST")):
                if o[k] is None:
                    assert r[col] == "", (key, col, r[col])
                else:
                    tol = 1e-12 + 1e-10 * abs(o[k]) if col == "FST" else None
                    assert abs(float(r[col]) - o[k]) <= tol if tol else gu.close(float(r[col]), o[k]), (key, col, r[col], o[k])
            if o["snp_count"] == 0:
                assert all(r[c] == "" for c in DV.KEYS + cli.P_COLS), key
            else:
                assert r["S_pop1"] != "" and (r["p_T2D"] != "") == (o["T2D"] is not None), key
    assert _read_csv(outs[0]) == _read_csv(both[1])


def test_cli_without_regions_is_the_parents_path(tmp_path):
    """Without --regions the CLI's files are those of the calls it made before the flag existed: multi_scan /
    multi_sliding_scan without a regions argument and write_csv, byte for byte."""
    import twoDSFS_class as T
    from sfs2d import cli
    from sfs2d.vcf import make_packed_vcf
    vcf, pm = _vcf()
    outs = cli.main([vcf, pm, "--window", "500000", "--fst", "--out-prefix", str(tmp_path / "X")])
    outs += cli.main([vcf, pm, "--window", "20000", "--step", "5000", "--fst", "--out-prefix", str(tmp_path / "X")])
    assert [os.path.basename(o) for o in outs] == ["X_500kb.csv", "X_20kb_step5kb.csv"]
    packed = make_packed_vcf(vcf, pm, "uv", "bv")
    obj = T.LikelihoodInference_jointSFS(vcf, pm)
    res = obj.multi_scan(packed, [500000], [], fst=True)
    cli.write_csv(str(tmp_path / "P_500kb.csv"), res[500000], {}, res["fst"][500000], None, False)
    rows = obj.multi_sliding_scan(packed, [20000], 5000, fst=True)[20000]
    cli.write_csv(str(tmp_path / "P_slide.csv"), rows, {}, {k: r["FST"] for k, r in rows.items()}, None, False)
    assert open(outs[0], "rb").read() == open(tmp_path / "P_500kb.csv", "rb").read()
    assert open(outs[1], "rb").read() == open(tmp_path / "P_slide.csv", "rb").read()
