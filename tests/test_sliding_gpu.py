"""Sliding plans (sfs2d_plan_create_sliding / sfs2d_plan_attach_sliding) against the oracle, window by window.

The expected windows are built here from the definition: for window W and step S (W % S == 0), a chromosome
with last position L has (L - 1) // S + 1 slots (one when L == 0); slot j holds the SNPs with
j S + 1 <= pos <= j S + W, begin = the first SNP with pos >= j S + 1 (slot 0: the chromosome's first SNP),
end = the first SNP with pos >= j S + W + 1 (np.searchsorted).  O.window_records / O.window_fst of the same
O.Cfg give each window's values: integers exact, T by golden_util.close with None exactly where the oracle
has None (sfs2d.post._v), Fst within 1e-12 + 1e-10 |x| (test_scan_variants' tolerance).

W = 6,400 bp; steps 6,400 / 1,600 / 100 (m = 1, 4, 64).  Chromosomes of LENGTHS SNPs under SFS2D_TILE = 4096:
one SNP (L < S, monomorphic: a None window), seven SNPs at 0, 1, S, S + 1, W, W + 1 and 2 W (L a multiple of
every step), and three dense ones (a window holds > 512 SNPs: k_scan_w's streamed rows) with SNPs exactly at
j S, j S + 1, j S + W and j S + W + 1 and, in the longest, a gap of more than two windows (empty slots in
mid-chromosome).  Every 37th SNP carries one of Fst's edge values, SNPs with fewer than 2 called alleles in a
population among them."""
import numpy as np
import pytest

import golden_util as gu
from oracle import sfs_oracle as O

pytestmark = pytest.mark.gpu

LENGTHS = [1, 7, 2049, 4097, 12300]
W = 6400
STEP = {1: 6400, 4: 1600, 64: 100}
VT = "intron_variant"
INTS = ("chrom", "wid", "begin", "end", "snp_count", "n2", "n2_all", "n1a", "n1b", "flags")
_DATA, _REF = {}, {}


@pytest.fixture(autouse=True)
def _small_tiles(monkeypatch):
    monkeypatch.setenv("SFS2D_TILE", "4096")
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------- data

def _positions(rng, n, span, special, gap=None):
    """n sorted distinct positions in [1, span): `special` among them, none inside `gap` = [lo, hi)."""
    free = np.setdiff1d(np.arange(1, span), np.asarray(special))
    if gap is not None:
        free = free[(free < gap[0]) | (free >= gap[1])]
    pos = np.concatenate([rng.choice(free, size=n - len(special), replace=False), special])
    pos.sort()
    assert len(np.unique(pos)) == n
    return pos


def _genome(n1p, n2p, chroms=None):
    """The genome at pop sizes (n1p, n2p); chroms: only those chromosomes of it."""
    key = (n1p, n2p)
    if chroms is not None:
        if key + (chroms,) not in _DATA:
            _DATA[key + (chroms,)] = _genome(n1p, n2p).subset_chroms(chroms)
        return _DATA[key + (chroms,)]
    if key in _DATA:
        return _DATA[key]
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(20 + n1p))
    n1, n2 = 2 * n1p, 2 * n2p
    S = STEP[4]
    edges = lambda j: [j * S, j * S + 1, j * S + W, j * S + W + 1]
    pos = [np.array([50]), np.array([0, 1, S, S + 1, W, W + 1, 2 * W]),
           _positions(rng, LENGTHS[2], 16000, edges(3)),
           _positions(rng, LENGTHS[3], 30000, edges(5)),
           # (j S for every step: 38,400 = 6 W, 40,000 = 25 * 1,600 = 400 * 100)
           _positions(rng, LENGTHS[4], 64000, edges(24) + edges(25), gap=(20001, 20001 + 2 * W + S))]
    assert [len(x) for x in pos] == LENGTHS
    counts, ann = [], []
    for x in pos:
        _, r1, a1, r2, a2 = synth_chrom(rng, len(x), n1p, n2p)
        counts.append(pack_counts(r1, a1, r2, a2))
        ann.append(rng.integers(0, 3, size=len(x)).astype(np.uint16))
    counts = np.concatenate(counts)
    counts[0] = int(pack_counts(np.array([n1]), np.array([0]), np.array([n2]), np.array([0]))[0])   # monomorphic
    h1, h2 = n1 // 2, n2 // 2
    edge = [(n1, 0, n2 - 1, 1), (n1 - 1, 1, n2, 0), (0, n1, h2, n2 - h2), (h1, n1 - h1, 0, n2), (0, n1, n2 - 1, 1),
            (n1, 0, 0, n2), (0, n1, n2, 0), (1, 1, h2, h2), (0, 2, h2 + 3, h2 - 3), (2, 0, 1, 1),
            (1, 0, h2, h2), (0, 1, h2, h2), (h1, h1, 0, 1), (0, 0, h2, h2), (h1, h1, 0, 0), (0, 1, 0, 1)]
    at = np.arange(11, len(counts), 37)
    e = np.array([edge[k % len(edge)] for k in range(len(at))])
    counts[at] = pack_counts(e[:, 0], e[:, 1], e[:, 2], e[:, 3])
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    p = PackedSNPs(counts, np.concatenate(pos).astype(np.uint32), off, [f"chr{i:04d}" for i in range(len(LENGTHS))],
                   np.concatenate(ann), ["intergenic_region", VT, "missense_variant"], "p1", "p2")
    _DATA[key] = p
    return p


def _slots(p, w, s):
    """Every slot of the sliding geometry, from the definition: [(chrom, j, begin, end)], begin == end empty."""
    out = []
    for c in range(p.nchrom):
        lo, hi = int(p.chrom_off[c]), int(p.chrom_off[c + 1])
        if lo == hi:
            continue
        pos = p.pos[lo:hi].astype(np.int64)
        last = int(pos[-1])
        js = np.arange((last - 1) // s + 1 if last else 1, dtype=np.int64)
        b = np.searchsorted(pos, js * s + 1, "left")
        b[0] = 0
        e = np.searchsorted(pos, js * s + w + 1, "left")
        out += [(c, int(j), lo + int(x), lo + int(max(x, y))) for j, x, y in zip(js, b, e)]
    return out


def _no_cancelled_t(values):
    """No oracle T in (0, 1e-2): below that the absolute rounding error of any evaluation order (~1e-12 on
    sums of terms up to ~2e4) passes 1e-10 relative (test_filtered_plans._no_cancelled_t)."""
    for v in values:
        assert v is None or v == 0.0 or not np.isfinite(v) or abs(v) >= 1e-2, v


def _oracle(n1p, n2p, m, vt=None, fold=True, start=None, bg_chrom=None, w=W, s=None, chroms=None):
    """(slots, records of the non-empty ones, their Fst), once per case; the fixture's properties asserted
    (chroms: a part of the genome, which need not hold the empty slots and the long windows)."""
    s = STEP[m] if s is None else s
    key = (n1p, n2p, w, s, vt, fold, start, bg_chrom, chroms)
    if key not in _REF:
        p = _genome(n1p, n2p, chroms)
        ocfg = O.Cfg(n1p, n2p, vt, fold, start, None)
        bgs = O.chrom_backgrounds(p, ocfg)
        slots = _slots(p, w, s)
        wins = [x for x in slots if x[2] < x[3]]
        recs = O.window_records(p, wins, ocfg, (lambda c: bgs[c]) if bg_chrom is None else (lambda c: bgs[bg_chrom]))
        fst = [O.window_fst(p, np.arange(x[2], x[3]), ocfg) for x in wins]
        _no_cancelled_t(o[t] for o in recs for t in ("T2D", "T1D_p1", "T1D_p2"))
        assert any(o["T2D"] is None for o in recs)                       # a None window
        assert any(o["T2D"] is not None and np.isfinite(o["T2D"]) for o in recs)
        assert max(x[3] - x[2] for x in wins) > 512                      # streamed rows
        mid = [i for i, x in enumerate(slots) if x[2] == x[3] and 0 < i < len(slots) - 1
               and slots[i - 1][0] == x[0] == slots[i + 1][0]]
        assert chroms is not None or (len(wins) < len(slots) and mid)    # empty slots, in mid-chromosome
        _REF[key] = (slots, recs, fst)
    return _REF[key]


# ------------------------------------------------------------------------------------------ checks

def _cfg(p, n1p, n2p, m=None, vt=None, fold=True, start=None, w=W, s=None, **kw):
    from sfs2d import _lib as L
    from sfs2d.engine import ScanConfig
    step = None if m is None and s is None else (STEP[m] if s is None else s)
    return ScanConfig(n1p=n1p, n2p=n2p, fold=fold, window_mode=L.WINDOW_BP, window=w, start_position=start,
                      ann_want=-1 if vt is None else p.ann_names.index(vt), step=step, **kw)


def _check(recs, fst, ref):
    from sfs2d import _lib as L
    from sfs2d import post
    slots, orec, ofst = ref
    assert len(recs) == len(slots), (len(recs), len(slots))
    assert fst is None or len(fst) == len(slots)
    k = 0
    for i, ((c, j, b, e), r) in enumerate(zip(slots, recs)):
        assert (int(r["chrom"]), int(r["wid"])) == (c, j), (i, c, j)
        if b == e:
            assert int(r["flags"]) & L.W_EMPTY and (int(r["begin"]), int(r["end"])) == (0, 0), (i, c, j)
            assert fst is None or np.isnan(fst[i]), (i, "fst of an empty slot")
            continue
        o = orec[k]
        assert not int(r["flags"]) & L.W_EMPTY and (int(r["begin"]), int(r["end"])) == (b, e), (i, c, j, b, e)
        for a, q in (("snp_count", "snp_count"), ("n2", "N2"), ("n2_all", "N2_all"), ("n1a", "N1a"), ("n1b", "N1b")):
            assert int(r[a]) == o[q], (i, a, int(r[a]), o[q])
        for which, q in ((2, "T2D"), (1, "T1D_p1"), (0, "T1D_p2")):
            v = post._v(r, which)
            assert (v is None) == (o[q] is None), (i, q, v, o[q])
            assert gu.close(v, o[q]), (i, q, v, o[q])
        if fst is not None:
            g, f = float(fst[i]), ofst[k]
            assert (np.isnan(g) if f is None else abs(g - f) <= 1e-12 + 1e-10 * abs(f)), (i, "fst", g, f)
        k += 1
    assert k == len(orec)


def _same_ints(a, b, fa=None, fb=None):
    for k in INTS:
        assert np.array_equal(a[k], b[k]), k
    if fa is not None:
        assert fa.tobytes() == fb.tobytes()


def _same_t(a, b):
    for k in ("t2d", "t1d_p1", "t1d_p2"):
        for x, y in zip(a[k], b[k]):
            assert gu.close(float(x), float(y)), (k, x, y)


def _run(p, cfg, bg=None, kernel=None):
    """run, then run_many(2): the records and Fst of both; the replay's integers and Fst are the first run's."""
    from sfs2d.engine import Engine
    eng = Engine.get(0)
    dev = eng.upload(p)
    pl = eng.plan(dev, cfg)
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
    finally:
        pl.close()
        dev.close()
    _same_ints(r0, r1, f0, f1)
    _same_t(r0, r1)
    return r0, f0


KERNELS = {"w_fused": (18, 14, {"SFS2D_FUSED": "1"}, "k_scan_w"), "w_sliced": (18, 14, {"SFS2D_FUSED": "0"}, "k_scan_w"),
           "gw": (50, 50, {"SFS2D_GW": "1"}, "k_scan_gw"), "g": (50, 50, {"SFS2D_GW": "0"}, "k_scan_g")}


# ------------------------------------------------------------------------------------------- tests

@pytest.mark.parametrize("m", [1, 4, 64])
@pytest.mark.parametrize("path", list(KERNELS))
def test_grids_and_steps(monkeypatch, path, m):
    """Per-chromosome backgrounds, folded, with Fst (summed by k_scan_w's scan; k_fst_win on the large grids),
    on every scan kernel at m = 1, 4, 64; the replay leaves the state clean.  m = 1: records and Fst are the
    ordinary plan's, byte for byte (the T values of the large-grid kernels by close: they are not reproducible
    to the last bit between two runs of one plan).  m = 4: the same plan without Fst has the same integers."""
    n1p, n2p, env, kernel = KERNELS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    # (the oracle costs ~6 ms per window on the 101 x 101 grid: its 64-step case scans the first three chromosomes,
    # ~290 windows; the empty slots of the longest one are in that grid's m = 1 and m = 4 cases)
    chroms = (0, 1, 2) if (m == 64 and n1p == 50) else None
    p = _genome(n1p, n2p, chroms)
    ref = _oracle(n1p, n2p, m, chroms=chroms)
    recs, fst = _run(p, _cfg(p, n1p, n2p, m, fst=True), kernel=kernel)
    _check(recs, fst, ref)
    if m == 1:
        plain, pf = _run(p, _cfg(p, n1p, n2p, None, fst=True), kernel=kernel)
        _same_ints(recs, plain, fst, pf)
        if kernel == "k_scan_w":
            assert recs.tobytes() == plain.tobytes()
        else:   # (eval_exact sums a bin's term in whichever lane takes the bin: on the large-grid kernels a T's last
                # bits differ between two runs of one and the same plan, test_filtered_plans.test_large_grids_filtered)
            _same_t(recs, plain)
    if m == 4:
        nof, _ = _run(p, _cfg(p, n1p, n2p, m), kernel=kernel)
        _check(nof, None, ref)
        _same_ints(recs, nof)


@pytest.mark.parametrize("case", ["supplied", "supplied_fst", "unfolded", "filtered_fused", "filtered_sliced",
                                  "filtered_nofst", "fst_win_counts", "supplied_gw"])
def test_backgrounds_and_filters(monkeypatch, case):
    """m = 4.  A supplied background (counts plans launch k_slots_slide and the scan alone), unfolded spectra,
    a start_position + variant_type filter on the bins pipeline (Fst by k_fst_win from the bins words, and
    without Fst), a counts plan whose Fst is k_fst_win's (SFS2D_FST_SCAN=0), a supplied background on
    k_scan_gw."""
    n1p, n2p = (50, 50) if case == "supplied_gw" else (18, 14)
    p = _genome(n1p, n2p)
    kw, okw, bg, kernel = {}, {}, None, "k_scan_gw" if case == "supplied_gw" else "k_scan_w"
    if case.startswith("supplied"):
        from sfs2d import _lib as L
        okw = dict(bg_chrom=4)
        kw = dict(bg_mode=L.BG_SUPPLIED, fst=case != "supplied")
        bg = O.chrom_backgrounds(p, O.Cfg(n1p, n2p))[4]
    elif case == "unfolded":
        okw = dict(fold=False)
        kw = dict(fold=False, fst=True)
    elif case.startswith("filtered"):
        start = int(p.pos[int(p.chrom_off[4]) + 4096 + 1])   # the second SNP of a lane's four, after a tile edge
        okw = dict(vt=VT, start=start)
        kw = dict(vt=VT, start=start, fst=case != "filtered_nofst")
        monkeypatch.setenv("SFS2D_FUSED", "0" if case == "filtered_sliced" else "1")
    else:
        monkeypatch.setenv("SFS2D_FST_SCAN", "0")
        kw = dict(fst=True)
    ref = _oracle(n1p, n2p, 4, **okw)
    recs, fst = _run(p, _cfg(p, n1p, n2p, 4, **kw), bg=bg, kernel=kernel)
    _check(recs, fst, ref)


@pytest.mark.parametrize("path", ["w_fused", "w_sliced", "gw"])
def test_attached_sliding_plans(monkeypatch, path):
    """A sliding plan (W, S = W / 4, Fst) attached to an ordinary base (window S) and to a sliding base
    (2 S by S): the standalone sliding plan's integers and Fst byte for byte, its T by close, and the
    oracle's; the sliding base's own records are the oracle's too.  Twice (the base's replay)."""
    from sfs2d.engine import Engine
    n1p, n2p, env, kernel = KERNELS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = _genome(n1p, n2p)
    S = STEP[4]
    ref = _oracle(n1p, n2p, 4)
    alone, alone_f = _run(p, _cfg(p, n1p, n2p, 4, fst=True), kernel=kernel)
    eng = Engine.get(0)
    dev = eng.upload(p)
    for base_cfg in (_cfg(p, n1p, n2p, w=S), _cfg(p, n1p, n2p, w=2 * S, s=S, fst=True)):
        base = eng.plan(dev, base_cfg)
        att = base.attach(_cfg(p, n1p, n2p, 4, fst=True))
        assert att.scan_kernel() == kernel
        for _ in range(2):
            base.run()
            base.check()
            att.check()
            recs, fst = att.read(), att.read_fst()
            _same_ints(recs, alone, fst, alone_f)
            _same_t(recs, alone)
            _check(recs, fst, ref)
        if base_cfg.step is not None:
            _check(base.read(), base.read_fst(), _oracle(n1p, n2p, None, w=2 * S, s=S))
        base.close()
    dev.close()


def test_streams_and_graph():
    """Two sliding plans round-robin on two streams (sfs2d_plan_run_streams), then captured and replayed
    (sfs2d_graph_*): each writes what the same plan writes run alone."""
    import torch
    from sfs2d import _lib as L
    from sfs2d.engine import Engine, Plan
    p = _genome(18, 14)
    cfg = _cfg(p, 18, 14, 4, fst=True)
    want, want_f = _run(p, cfg, kernel="k_scan_w")
    _check(want, want_f, _oracle(18, 14, 4))
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
            _same_ints(got, want, q.read_fst(), want_f)
            _same_t(got, want)

    Plan.run_streams(plans, streams, 5, optrs)
    check_all()
    g = Plan.graph(plans, streams, 4, optrs)
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    g.launch(2)
    check_all()
    g.close()
    for q in plans:
        q.close()
    dev.close()


def test_refusals():
    """W % S != 0, m = 65, SNP-count windows and prev_extra: Sfs2dError with a message, for standalone and
    attached sliding plans; an ordinary plan on the same ctx afterwards still matches the oracle."""
    from sfs2d import _lib as L
    from sfs2d.engine import Engine
    p = _genome(18, 14)
    eng = Engine.get(0)
    dev = eng.upload(p)
    base = eng.plan(dev, _cfg(p, 18, 14, w=STEP[4]))
    bad = [_cfg(p, 18, 14, s=1500), _cfg(p, 18, 14, w=6500, s=100), _cfg(p, 18, 14, s=0), _cfg(p, 18, 14, s=2 * W),
           _cfg(p, 18, 14, 4, prev_extra=True)]
    snp = _cfg(p, 18, 14, w=64, s=16)
    snp.window_mode = L.WINDOW_SNPS
    for cfg in bad + [snp]:
        for make in (lambda c: eng.plan(dev, c), base.attach):
            with pytest.raises(L.Sfs2dError) as ei:
                make(cfg)
            assert ei.value.code == L.E_ARG and len(str(ei.value)) > len("sfs2d error -1: "), str(ei.value)
    base.close()
    dev.close()
    recs, fst = _run(p, _cfg(p, 18, 14, None, fst=True), kernel="k_scan_w")
    _check(recs, fst, _oracle(18, 14, 1))


def _clean_rows(p, ref, w, s, fst):
    """The rows post.sliding_scan is specified to build, from the oracle's records."""
    slots, orec, ofst = ref
    rows = {}
    for (c, j, b, e), o, f in zip([x for x in slots if x[2] < x[3]], orec, ofst):
        t2, t1, tb = o["T2D"], o["T1D_p1"], o["T1D_p2"]
        row = {"snp_count": o["snp_count"], "T2D": t2, "T1D_pop1": t1, "T1D_pop2": tb,
               "new_term_pop1": None if t2 is None or t1 is None else t2 - t1,
               "new_term_pop2": None if t2 is None or tb is None else t2 - tb,
               "T2D_diff": None if None in (t2, t1, tb) else t2 - (t1 + tb) / 2}
        if fst:
            row["FST"] = f
        rows[f"{p.chrom_names[c]} {j * s + 1}-{j * s + w}"] = row
    return rows


def _compare_rows(got, want):
    for k in want:
        if "FST" in want[k]:
            g, f = got[k].pop("FST"), want[k]["FST"]
            assert (g is None) if f is None else abs(g - f) <= 1e-12 + 1e-10 * abs(f), (k, g, f)
    want = {k: {a: b for a, b in r.items() if a != "FST"} for k, r in want.items()}
    assert gu.compare_results(got, want) == []


def test_class_methods():
    """LikelihoodInference_jointSFS.sliding_scan (per-chromosome and a named background chromosome) and
    multi_sliding_scan against rows built from the oracle's records by the clean rule."""
    import twoDSFS_class as T
    p = _genome(18, 14)
    S = STEP[4]
    obj = T.LikelihoodInference_jointSFS(None, None, pop1=p.pop1, pop2=p.pop2, pop1_size=18, pop2_size=14)
    _compare_rows(obj.sliding_scan(p, W, S, fst=True), _clean_rows(p, _oracle(18, 14, 4), W, S, True))
    _compare_rows(obj.sliding_scan(p, W, S, background_chromosome="chr0004"),
                  _clean_rows(p, _oracle(18, 14, 4, bg_chrom=4), W, S, False))
    with pytest.raises(ValueError, match="Background chromosome nope not found in the data."):
        obj.sliding_scan(p, W, S, background_chromosome="nope")
    multi = obj.multi_sliding_scan(p, [W, 2 * S], S, fst=True)
    assert list(multi) == [2 * S, W]
    _compare_rows(multi[W], _clean_rows(p, _oracle(18, 14, 4), W, S, True))
    _compare_rows(multi[2 * S], _clean_rows(p, _oracle(18, 14, None, w=2 * S, s=S), 2 * S, S, True))


def test_cli_step(tmp_path):
    """python -m sfs2d VCF POPMAP --window 20000 --step 5000 --fst: <prefix>_20kb_step5kb.csv with the existing
    columns + FST, its rows sliding_scan(..., fst=True)'s; the windows at j = 0 (mod 4) are the disjoint 20 kb
    windows: their snp_count and Fst are the ordinary scan's (window_fst and the oracle's segmentation)."""
    import csv
    import os
    import twoDSFS_class as T
    from sfs2d import cli
    from sfs2d.vcf import read_vcf
    vcf, pm = os.path.join(gu.GOLD, "vcf_test.vcf.gz"), os.path.join(gu.GOLD, "popmap_ref.txt")
    outs = cli.main([vcf, pm, "--window", "20000", "--step", "5000", "--fst", "--out-prefix", str(tmp_path / "X")])
    assert [os.path.basename(o) for o in outs] == ["X_20kb_step5kb.csv"]
    with open(outs[0], newline="") as fh:
        rows = list(csv.DictReader(fh))
    assert list(rows[0]) == T.col_names + ["FST"]
    p = read_vcf(vcf, pm).to_packed("uv", "bv")
    obj = T.LikelihoodInference_jointSFS(vcf, pm)
    want = obj.sliding_scan(p, 20000, 5000, fst=True)
    assert [f"{r['chromosome']} {r['window_start']}-{r['window_end']}" for r in rows] == list(want)
    txt = lambda v: "" if v is None else str(v)
    for r, o in zip(rows, want.values()):
        assert r["snp_count"] == str(o["snp_count"]) and r["FST"] == txt(o["FST"])
        assert (r["T2D"], r["T1D_p1"], r["T2D_diff"]) == (txt(o["T2D"]), txt(o["T1D_pop1"]), txt(o["T2D_diff"]))
    plain_fst = obj.window_fst(p, window_size=20000)
    plain_n = {f"{p.chrom_names[c]} {s}-{s + 19999}": e - b for c, s, b, e in O.bp_windows(p, 20000)}
    on_grid = {k: o for k, o in want.items() if (int(k.split(" ")[1].split("-")[0]) - 1) % 20000 == 0}
    assert list(on_grid) == list(plain_fst) == list(plain_n) and len(on_grid) > 3
    for k, o in on_grid.items():
        f = plain_fst[k]
        assert o["snp_count"] == plain_n[k], k
        assert (o["FST"] is None) if f is None else abs(o["FST"] - f) <= 1e-12 + 1e-10 * abs(f), (k, o["FST"], f)
