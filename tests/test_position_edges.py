"""The position axis at its edges, against the oracle window by window (wide_util.check_records: integers exact,
T by golden_util.close, Fst within 1e-12 + 1e-10 |x| unless a test says otherwise).

Duplicate positions: sfs2d_data_upload clears `strict` on pos[i] <= pos[i-1]; plan_create then derives the bin
width, the largest window and the Fst fixed point from the longest run of the host positions (its sliding
branch from a two-pointer bound).  dup_genome() holds runs of 2 to 40 equal positions on ~30% of the positions and
one run of 5,000, scanned under SFS2D_TILE=2048 (a run covers SNP 2048: k_prep's tile edge, a step edge and a
multiple of 4 and 64 at once).

Position 0 and the top of uint32: edge_genome()'s first chromosome starts 0, 0, 1 and ends 4294967290,
4294967295, 4294967295, with SNPs on both sides of every multiple of the window sizes below 2^32 that the fixture
names; the window-id arithmetic (div_magic / wid_fast in k_prep, the 64-bit bounds of k_slots_bp / k_slots_search /
k_slots_slide, window_begin_back, the host's slot_base) sees dividends up to 2^32 - 2 and window sizes from 65,536
(65,536 slots) to 2^32 - 1.

Counts past the ln table (LNX_N = 2^20): million_genome() has a window, a window bin, a background and a
background bin of 2^20 + 100 SNPs or more."""
import numpy as np
import pytest

import wide_util as U
from oracle import sfs_oracle as O

pytestmark = pytest.mark.gpu

VT = "intron_variant"
DUP_WS, DUP_TILE = 20000, 2048
EDGE_WS = [65536, 65537, 1000003, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 3 * 2 ** 30, 2 ** 32 - 1]
EDGE_SNPS = [1, 2, 63, 64, 65]   # + len(chromosome 0)
MILLION, MILLION_WS = 2 ** 20 + 100, 300000
_DATA, _BG = {}, {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE", "SFS2D_WGS", "SFS2D_LNL"):
        monkeypatch.delenv(k, raising=False)


def _cfg(p, n1p, n2p, window, vt=None, bg=False, **kw):
    from sfs2d import _lib as L
    from sfs2d.engine import ScanConfig
    return ScanConfig(n1p=n1p, n2p=n2p, window=window, ann_want=-1 if vt is None else p.ann_names.index(vt),
                      bg_mode=L.BG_SUPPLIED if bg else L.BG_PER_CHROM, **kw)


def _bgs(name, p, ocfg):
    key = (name, ocfg.n1p, ocfg.n2p, ocfg.variant_type)
    if key not in _BG:
        _BG[key] = O.chrom_backgrounds(p, ocfg)
    return _BG[key]


def _run(p, cfg, bg=None):
    from sfs2d.engine import Engine
    dev = Engine.get(0).upload(p)
    try:
        return U.run_plan(dev, cfg, bg)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------- duplicate positions

def run_lengths(pos):
    """Lengths of the runs of equal values of a sorted array, and each run's first index."""
    first = np.flatnonzero(np.concatenate([[True], pos[1:] != pos[:-1]]))
    return np.diff(np.concatenate([first, [len(pos)]])), first


def dup_genome(n1p=25, n2p=25):
    """Three chromosomes of 2,600 / 6,400 / 300 SNPs: 70% of the positions hold one SNP, the others runs of 2 to
    40 SNPs; the middle of chromosome 1 is one run of 5,000.  The distinct positions are synth_chrom's with a mean
    gap of 400 bp (~7 SNPs per position: the ordinary SNP density)."""
    key = ("dup", n1p, n2p)
    if key in _DATA:
        return _DATA[key]
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(4040))
    counts, pos, ann, off = [], [], [], [0]
    for n, big in ((2600, 0), (1400, 5000), (300, 0)):
        runs = []
        while sum(runs) < n:
            runs.append(1 if rng.random() < 0.7 else int(rng.integers(2, 41)))
        runs[-1] -= sum(runs) - n
        if big:
            runs.insert(len(runs) // 2, big)
        distinct, r1, a1, r2, a2 = synth_chrom(rng, len(runs), n1p, n2p, mean_gap=400.0)
        pos.append(np.repeat(distinct, runs))
        _, r1, a1, r2, a2 = synth_chrom(rng, n + big, n1p, n2p)
        counts.append(pack_counts(r1, a1, r2, a2))
        ann.append(rng.integers(0, 3, size=n + big).astype(np.uint16))
        off.append(off[-1] + n + big)
    _DATA[key] = PackedSNPs(np.concatenate(counts), np.concatenate(pos).astype(np.uint32), np.array(off, np.int64),
                            ["chr0000", "chr0001", "chr0002"], np.concatenate(ann),
                            ["intergenic_region", VT, "missense_variant"], "p1", "p2")
    return _DATA[key]


def dup_ref(n1p, n2p, window, vt=None, step=None, attach=False):
    """(data, oracle Cfg, backgrounds, reference) of the duplicate-position genome at one window geometry."""
    p = dup_genome(n1p, n2p)
    ocfg = O.Cfg(n1p, n2p, vt)
    bgs = _bgs("dup", p, ocfg)
    if step:
        wins = [s for s in U.sliding_slots(p, window, step) if s[2] < s[3]]
    else:
        wins = O.bp_windows(p, window)
    return p, ocfg, bgs, U.oracle_ref(p, wins, ocfg, lambda c: bgs[c], key=("dup", n1p, n2p, window, vt, step))


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "sliced"])
@pytest.mark.parametrize("fst", [True, False], ids=["fst", "nofst"])
def test_duplicates_fixed_bp(monkeypatch, fused, fst):
    monkeypatch.setenv("SFS2D_TILE", str(DUP_TILE))
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    p, ocfg, bgs, ref = dup_ref(25, 25, DUP_WS)
    recs, f, v = _run(p, _cfg(p, 25, 25, DUP_WS, fst=fst))
    assert (v["p16"], v["fused"], v["cnt"]) == (1, fused, 1), v
    U.check_records(recs, f, ref)


def test_duplicates_bins_plan(monkeypatch):
    monkeypatch.setenv("SFS2D_TILE", str(DUP_TILE))
    p, ocfg, bgs, ref = dup_ref(25, 25, DUP_WS, vt=VT)
    recs, f, v = _run(p, _cfg(p, 25, 25, DUP_WS, vt=VT, fst=True))
    assert v["cnt"] == 0, v
    U.check_records(recs, f, ref)


def test_duplicates_prev_extra(monkeypatch):
    """window_begin_back over runs of equal positions: the Q9 helper's window is the oracle's last but one."""
    import fake_records as FR
    import golden_util as gu
    from sfs2d import _lib as L
    monkeypatch.setenv("SFS2D_TILE", str(DUP_TILE))
    p, ocfg, bgs, ref = dup_ref(25, 25, DUP_WS)
    recs, _, _ = _run(p, _cfg(p, 25, 25, DUP_WS, prev_extra=True))
    U.check_records(recs, None, ref)
    want = FR.bp_records(p, DUP_WS, ocfg, lambda c: bgs[c], prev_extra=True)
    assert len(recs) == len(want)
    x, y = recs[-1], want[-1]
    assert int(x["flags"]) & L.W_EXTRA and not int(x["flags"]) & L.W_EMPTY
    for k in ("chrom", "begin", "end", "snp_count", "n2", "n2_all", "n1a", "n1b"):
        assert int(x[k]) == int(y[k]), (k, int(x[k]), int(y[k]))
    for k in ("t2d", "t1d_p1", "t1d_p2"):
        assert gu.close(float(x[k]), float(y[k])), (k, float(x[k]), float(y[k]))


@pytest.mark.parametrize("fst_scan", [True, False], ids=["fst_in_scan", "fst_win"])
def test_duplicates_sliding(monkeypatch, fst_scan):
    """The sliding branch's two-pointer bound on non-strict positions; windows from the definition."""
    monkeypatch.setenv("SFS2D_TILE", str(DUP_TILE))
    if not fst_scan:
        monkeypatch.setenv("SFS2D_FST_SCAN", "0")
    p, ocfg, bgs, ref = dup_ref(25, 25, DUP_WS, step=DUP_WS // 4)
    recs, f, _ = _run(p, _cfg(p, 25, 25, DUP_WS, fst=True, step=DUP_WS // 4))
    slots = U.sliding_slots(p, DUP_WS, DUP_WS // 4)
    assert len(recs) == len(slots) and [int(r["wid"]) for r in recs] == [s[1] for s in slots]
    U.check_records(recs, f, ref)


def test_duplicates_attached(monkeypatch):
    """A 20 kb base with an attached 100 kb plan (k_slots_bp's searches on runs of equal positions)."""
    from sfs2d.engine import Engine
    monkeypatch.setenv("SFS2D_TILE", str(DUP_TILE))
    p, ocfg, bgs, ref = dup_ref(25, 25, DUP_WS)
    _, _, _, ref5 = dup_ref(25, 25, 5 * DUP_WS)
    dev = Engine.get(0).upload(p)
    base = None
    try:
        base = dev.eng.plan(dev, _cfg(p, 25, 25, DUP_WS, fst=True))
        att = base.attach(_cfg(p, 25, 25, 5 * DUP_WS, fst=True))
        base.run()
        base.check()
        out = [(q.read(), q.read_fst()) for q in (base, att)]
    finally:
        if base is not None:
            base.close()
        dev.close()
    U.check_records(out[0][0], out[0][1], ref)
    U.check_records(out[1][0], out[1][1], ref5)


def test_duplicates_supplied_background(monkeypatch):
    """A counts plan with a supplied background takes its slots from k_slots_search, with SFS2D_SEG=prep from
    k_prep's segmentation: identical records, both the oracle's."""
    monkeypatch.setenv("SFS2D_TILE", str(DUP_TILE))
    p = dup_genome()
    ocfg = O.Cfg(25, 25)
    bg = _bgs("dup", p, ocfg)[0]
    wins = O.bp_windows(p, DUP_WS)
    cfg = _cfg(p, 25, 25, DUP_WS, bg=True)
    recs, _, v = _run(p, cfg, bg)
    assert (v["fused"], v["cnt"]) == (0, 1), v
    monkeypatch.setenv("SFS2D_SEG", "prep")
    recs2, _, _ = _run(p, cfg, bg)
    assert recs.tobytes() == recs2.tobytes()
    U.check_against_oracle(recs, None, p, wins, ocfg, lambda c: bg, key=("dup-sup", DUP_WS))


@pytest.mark.parametrize("gw", [1, 0])
def test_duplicates_large_grid(monkeypatch, gw):
    monkeypatch.setenv("SFS2D_TILE", str(DUP_TILE))
    monkeypatch.setenv("SFS2D_GW", str(gw))
    p, ocfg, bgs, ref = dup_ref(50, 50, DUP_WS)
    recs, f, v = _run(p, _cfg(p, 50, 50, DUP_WS, fst=True))
    assert v["fused"] == -1 and v["tri"] == (1 if gw else -1), v
    U.check_records(recs, f, ref)


def test_duplicates_window_of_7_bp(monkeypatch):
    """window = 7: most windows hold one position's run (a window's first and last SNP share a position)."""
    monkeypatch.setenv("SFS2D_TILE", str(DUP_TILE))
    p, ocfg, bgs, ref = dup_ref(25, 25, 7)
    recs, f, _ = _run(p, _cfg(p, 25, 25, 7, fst=True))
    assert len(recs) < 65536
    U.check_records(recs, f, ref)


# ------------------------------------------------------------------------------------------- position 0 .. 2^32 - 1

def edge_genome():
    """Chromosome 0: 2,000 SNPs at 0, 0, 1, ..., 4294967290, 4294967295, 4294967295; in between, SNPs at m - 1, m,
    m + 1 and m + 2 for every multiple m < 2^32 - 2 of a window size of EDGE_WS that is one of the first three, a
    power-of-two neighbour or 3 2^30, and 24 clusters of ordinary density spread over the axis (most of it is
    empty slots).  Chromosome 1: 400 ordinary SNPs."""
    if "edge" in _DATA:
        return _DATA["edge"]
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(3232))
    marks = [65536, 65537, 2 * 65536, 2 * 65537, 1000003, 2 * 1000003, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 3 * 2 ** 30,
             2 ** 32 - 2 - (2 ** 32 - 2) % 65536, 2 ** 32 - 2 - (2 ** 32 - 2) % 65537]
    fixed = {0, 1, 4294967290, 4294967295}
    for m in marks:
        fixed.update(range(m - 1, m + 3))
    free = 2000 - 2 - len(fixed)   # (0 and 4294967295 twice)
    bases = np.sort(rng.integers(10 ** 6, 2 ** 32 - 10 ** 6, size=24))
    cl = np.concatenate([b + np.cumsum(1 + rng.integers(0, 110, size=free // 24 + 8)) for b in bases])
    cl = np.setdiff1d(cl, np.array(sorted(fixed)))[:free]
    pos0 = np.sort(np.concatenate([np.array(sorted(fixed)), cl, [0, 4294967295]]).astype(np.int64))
    assert len(pos0) == 2000 and pos0[-1] == 4294967295
    _, r1, a1, r2, a2 = synth_chrom(rng, 2000, 25, 25)
    pos1, s1, b1, s2, b2 = synth_chrom(rng, 400, 25, 25)
    counts = np.concatenate([pack_counts(r1, a1, r2, a2), pack_counts(s1, b1, s2, b2)])
    _DATA["edge"] = PackedSNPs(counts, np.concatenate([pos0, pos1]).astype(np.uint32), np.array([0, 2000, 2400], np.int64),
                               ["chr0000", "chr0001"], np.zeros(2400, np.uint16), ["intergenic_region"], "p1", "p2")
    return _DATA["edge"]


def edge_ref(window, snps=False, step=None):
    p = edge_genome()
    ocfg = O.Cfg(25, 25)
    bgs = _bgs("edge", p, ocfg)
    if step:
        wins = [s for s in U.sliding_slots(p, window, step) if s[2] < s[3]]
    else:
        wins = O.snp_windows(p, window)[0] if snps else O.bp_windows(p, window)
    return p, ocfg, bgs, U.oracle_ref(p, wins, ocfg, lambda c: bgs[c], key=("edge", window, snps, step))


@pytest.mark.parametrize("k", range(len(EDGE_WS)), ids=[str(w) for w in EDGE_WS])
def test_edges_fixed_bp(k):
    """Per window size: a per-chromosome plan with the Q9 helper (k_prep's segmentation: wid_fast;
    window_begin_back), the plan of the next size attached to it (k_slots_bp) and a supplied-background counts
    plan (k_slots_search)."""
    import fake_records as FR
    import golden_util as gu
    from sfs2d import _lib as L
    from sfs2d.engine import Engine
    ws, ws2 = EDGE_WS[k], EDGE_WS[(k + 1) % len(EDGE_WS)]
    p, ocfg, bgs, ref = edge_ref(ws)
    _, _, _, ref2 = edge_ref(ws2)
    dev = Engine.get(0).upload(p)
    base = sup = None
    try:
        base = dev.eng.plan(dev, _cfg(p, 25, 25, ws, fst=True, prev_extra=True))
        att = base.attach(_cfg(p, 25, 25, ws2, fst=True))
        base.run()
        base.check()
        out = [(q.read(), q.read_fst()) for q in (base, att)]
        sup = dev.eng.plan(dev, _cfg(p, 25, 25, ws, bg=True))
        sup.set_background(*bgs[1])
        sup.run()
        sup.check()
        srec = sup.read()
    finally:
        for q in (base, sup):
            if q is not None:
                q.close()
        dev.close()
    U.check_records(out[0][0], out[0][1], ref)
    U.check_records(out[1][0], out[1][1], ref2)
    last = int(p.pos[1999])
    assert len(out[0][0]) == (last - 1) // ws + 1 + (int(p.pos[-1]) - 1) // ws + 1 + 1
    want = FR.bp_records(p, ws, ocfg, lambda c: bgs[c], prev_extra=True)
    x, y = out[0][0][-1], want[-1]
    assert int(x["flags"]) & L.W_EXTRA
    for f in ("chrom", "begin", "end", "snp_count", "n2", "n2_all", "n1a", "n1b"):
        assert int(x[f]) == int(y[f]), (f, int(x[f]), int(y[f]))
    for f in ("t2d", "t1d_p1", "t1d_p2"):
        assert gu.close(float(x[f]), float(y[f])), (f, float(x[f]), float(y[f]))
    U.check_against_oracle(srec, None, p, ref[0], ocfg, lambda c: bgs[1], key=("edge-sup", ws))


def test_edges_sliding():
    """k_slots_slide's 64-bit bounds: ws = 2^31, step = 2^29 (8 slots; j step + ws + 1 passes 2^32)."""
    ws, step = 2 ** 31, 2 ** 29
    p, ocfg, bgs, ref = edge_ref(ws, step=step)
    recs, f, _ = _run(p, _cfg(p, 25, 25, ws, fst=True, step=step))
    slots = U.sliding_slots(p, ws, step)
    assert len([s for s in slots if s[0] == 0]) == 8
    assert len(recs) == len(slots) and [int(r["wid"]) for r in recs] == [s[1] for s in slots]
    U.check_records(recs, f, ref)


def test_edges_labels():
    """The window labels of combined_scan (one size) and sliding_scan through the drop-in class."""
    import golden_util as gu
    import twoDSFS_class as T
    p = edge_genome()
    obj = T.LikelihoodInference_jointSFS(None, None, pop1="p1", pop2="p2", pop1_size=25, pop2_size=25)
    ws = 2 ** 31 + 1
    assert gu.compare_results(obj.combined_scan(p, ws), O.combined_scan(p, ws, O.Cfg(25, 25))) == []
    ws, step = 2 ** 31, 2 ** 29
    got = obj.sliding_scan(p, ws, step)
    slots = [s for s in U.sliding_slots(p, ws, step) if s[2] < s[3]]
    assert list(got) == [f"{p.chrom_names[c]} {j * step + 1}-{j * step + ws}" for c, j, _, _ in slots]
    assert [r["snp_count"] for r in got.values()] == [e - b for _, _, b, e in slots]


@pytest.mark.parametrize("S", EDGE_SNPS + [2000])
def test_edges_snp_windows(S):
    """SNP-count windows of 1, 2, 63, 64, 65 SNPs and of the whole chromosome (div_fast's shift edge cases)."""
    from sfs2d import _lib as L
    p, ocfg, bgs, ref = edge_ref(S, snps=True)
    recs, f, _ = _run(p, _cfg(p, 25, 25, S, fst=True, window_mode=L.WINDOW_SNPS))
    assert len(recs) == 2000 // S + 400 // S
    assert [int(r["wid"]) for r in recs] == [(w[3] - int(p.chrom_off[w[0]])) // S for w in ref[0]]
    U.check_records(recs, f, ref)


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "sliced"])
def test_tiny_windows_other_fst_paths(monkeypatch, fused):
    """Windows of one or two SNPs, or of one position's run, in which every SNP is fixed for the alternative
    allele have no qualifying SNP: Fst is NaN on every path -- here SFS2D_FST_SCAN=0: k_prep's fixed-point sums
    (fused, SNP-count windows) and k_fst_win's floating-point sums (sliced fixed-bp windows); the tests above run
    the scan's own sums, which gave 1.0 and 2.0 for such windows (p = a * (1 / n) is not exactly 1)."""
    from sfs2d import _lib as L
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    monkeypatch.setenv("SFS2D_FST_SCAN", "0")
    for S in (1, 2):
        p, ocfg, bgs, ref = edge_ref(S, snps=True)
        assert any(f is None and o["N1a"] > 0 for f, o in zip(ref[2], ref[1]))
        recs, f, _ = _run(p, _cfg(p, 25, 25, S, fst=True, window_mode=L.WINDOW_SNPS))
        U.check_records(recs, f, ref)
    monkeypatch.setenv("SFS2D_TILE", str(DUP_TILE))
    p, ocfg, bgs, ref = dup_ref(25, 25, 7)
    assert any(f is None and o["N1a"] > 0 for f, o in zip(ref[2], ref[1]))
    recs, f, _ = _run(p, _cfg(p, 25, 25, 7, fst=True))
    U.check_records(recs, f, ref)


def test_edges_window_of_1_bp_is_refused():
    """window = 1 on this data is 2^32 - 1 slots: SFS2D_E_ARG with a message, nothing allocated."""
    from sfs2d import _lib as L
    from sfs2d.engine import Engine
    p = edge_genome()
    dev = Engine.get(0).upload(p)
    try:
        with pytest.raises(L.Sfs2dError, match="too many window slots") as ei:
            dev.eng.plan(dev, _cfg(p, 25, 25, 1))
        assert ei.value.code == L.E_ARG
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------- counts past the ln table

def million_genome(n1p=25, n2p=25):
    """Chromosome 0: 3,000 mixed SNPs (below 300,000 bp: window 0), 2^20 + 100 SNPs of one counts word at 4 per
    position from 300,001 on (window 1), then 3,000 mixed SNPs from 590,000 on (the first ~180 in window 1, the rest
    in window 2); chromosome 1: 3,000 ordinary SNPs (one window)."""
    key = ("million", n1p, n2p)
    if key in _DATA:
        return _DATA[key]
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(2020 + n1p))
    pos0, r1, a1, r2, a2 = synth_chrom(rng, 6000, n1p, n2p)
    mixed = pack_counts(r1, a1, r2, a2)
    word = int(pack_counts(np.array([2 * n1p - 3]), np.array([3]), np.array([2 * n2p - 20]), np.array([20]))[0])
    pos1, s1, b1, s2, b2 = synth_chrom(rng, 3000, n1p, n2p)
    counts = np.concatenate([mixed[:3000], np.full(MILLION, word, np.uint32), mixed[3000:], pack_counts(s1, b1, s2, b2)])
    pos = np.concatenate([pos0[:3000], 300001 + np.arange(MILLION) // 4, 590000 + (pos0[3000:] - pos0[3000]), pos1])
    assert pos0[2999] <= 300000 and 300001 + (MILLION - 1) // 4 < 590000
    n0 = 6000 + MILLION
    _DATA[key] = PackedSNPs(counts, pos.astype(np.uint32), np.array([0, n0, n0 + 3000], np.int64), ["chr0000", "chr0001"],
                            np.zeros(n0 + 3000, np.uint16), ["intergenic_region"], "p1", "p2")
    return _DATA[key]


def million_ref(n1p=25, n2p=25):
    p = million_genome(n1p, n2p)
    ocfg = O.Cfg(n1p, n2p)
    bgs = _bgs("million", p, ocfg)
    wins = O.bp_windows(p, MILLION_WS)
    return p, ocfg, bgs, U.oracle_ref(p, wins, ocfg, lambda c: bgs[c], key=("million", n1p, n2p))


def fst_fixed_point_bound(p, wins, ocfg):
    """The Fst error k_prep's fixed-point sums allow, per window.  plan_create scales each SNP's num and den by
    2^e, e = max(8, min(48, 61 - bitlen(maxsnp))), maxsnp the most SNPs of any window, and each term is rounded to
    an integer: either sum of a window of N SNPs is off by at most d = N 2^-(e+1).  With n = sum(num) and
    D = sum(den) of the oracle, |(n + dn) / (D + dD) - n / D| <= d (1 + |n / D|) / (D - d)."""
    maxsnp = max(w[-1] - w[-2] for w in wins)
    e = max(8, min(48, 61 - int(maxsnp).bit_length()))
    out = []
    for w in wins:
        idx = np.arange(w[-2], w[-1])
        r1, a1, r2, a2 = (x[idx].astype(np.float64) for x in (p.ref1, p.alt1, p.ref2, p.alt2))
        n1c, n2c = r1 + a1, r2 + a2
        p1, p2 = a1 / n1c, a2 / n2c
        num = (p1 - p2) ** 2 - p1 * (1 - p1) / (n1c - 1) - p2 * (1 - p2) / (n2c - 1)
        den = p1 * (1 - p2) + p2 * (1 - p1)
        n, D = float(num.sum()), float(den.sum())
        d = len(idx) * 2.0 ** -(e + 1)
        out.append(d * (1 + abs(n / D)) / (D - d))
    return e, out


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "sliced"])
def test_million_snp_bin_fst_in_scan(monkeypatch, fused):
    """N, B, a window bin and a background bin of >= 2^20 (lnx_of's log branch, k_bg_slice's, 2 (S - N ln N) past
    LNX_N); Fst summed in floating point by the scan: 1e-12 + 1e-10 |x|.  T under the `wide` rule."""
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    p, ocfg, bgs, ref = million_ref()
    recs, f, v = _run(p, _cfg(p, 25, 25, MILLION_WS, fst=True))
    assert v == dict(p16=0, fused=fused, fst=2, cnt=1, gate=1, tri=-1), v
    U.check_records(recs, f, ref, wide=True)


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "sliced"])
def test_million_snp_bin_fst_fixed_point(monkeypatch, fused):
    """SFS2D_FST_SCAN=0: Fst from k_prep's fixed-point sums (fused) / k_bg_slice's Fst workgroups (sliced, fp64
    sums), at e = 40 (maxsnp = 2^20 + 100 + ~180).  fst_fixed_point_bound for the big window (Fst = 0.266):
    1.4e-12 absolute; observed on the MI355X 2.6e-14 (fused), 3.7e-14 (sliced); the ordinary windows: bound
    2.3e-12, observed <= 3.0e-14."""
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    monkeypatch.setenv("SFS2D_FST_SCAN", "0")
    p, ocfg, bgs, ref = million_ref()
    e, bound = fst_fixed_point_bound(p, ref[0], ocfg)
    assert e == 40
    recs, f, v = _run(p, _cfg(p, 25, 25, MILLION_WS, fst=True))
    assert (v["p16"], v["fst"]) == (0, 1 if fused else 0), v
    _report(recs, f, ref, bound)
    U.check_records(recs, f, ref, wide=True, fst_tol=lambda i: bound[i])


@pytest.mark.parametrize("gw", [1, 0])
def test_million_snp_bin_large_grid(monkeypatch, gw):
    """50 x 50: k_scan_gw / k_scan_g with 32-bit bins, Fst from k_prep's fixed-point sums (same bound): 2.3e-12
    absolute for the big window (Fst = 0.124); observed on the MI355X 4.0e-13, both kernels."""
    monkeypatch.setenv("SFS2D_GW", str(gw))
    p, ocfg, bgs, ref = million_ref(50, 50)
    e, bound = fst_fixed_point_bound(p, ref[0], ocfg)
    recs, f, v = _run(p, _cfg(p, 50, 50, MILLION_WS, fst=True))
    assert (v["p16"], v["fst"], v["tri"]) == (0, 1, 1 if gw else -1), v
    _report(recs, f, ref, bound)
    U.check_records(recs, f, ref, wide=True, fst_tol=lambda i: bound[i])


def _report(recs, f, ref, bound):
    """Print each window's Fst error beside its bound (pytest -s)."""
    from sfs2d import _lib as L
    live = (recs["flags"][: len(f)] & L.W_EMPTY) == 0
    for (w, g, o, b) in zip(ref[0], f[live], ref[2], bound):
        print(f"fst window {w}: got {g!r} oracle {o!r} abs err {abs(g - o):.3e} bound {b:.3e} rel err {abs(g - o) / abs(o):.3e}")
