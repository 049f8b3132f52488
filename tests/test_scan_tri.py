"""k_scan_wt -- k_scan_w's lean variants on a triangle-packed window histogram, with batches of 32 windows and 8
lane copies of the 1D window histograms -- against the lean variants (SFS2D_TRI=0 at plan creation), against its
own A/B arms (SFS2D_SB=8, SFS2D_R1=4) and against the oracle.

Every comparison between two builds of one plan is of bytes (the 64-B records) and bits (Fst, NaNs included): the
packing moves histogram words, the batch size moves the place of a flush and the copies split integer counts, so no
floating-point sum changes its order.  The oracle comparisons use test_scan_lean.py's tolerance
(wide_util.check_records: integers exact, T by golden_util.close, Fst within 1e-12 + 1e-10 |x|).

Plan.scan_packing() reports {"tri", "sb", "r1"}; Plan.scan_variant() reports a packed plan as the lean (gated)
variant it equals, as it reports a lean one.  "The new default" of a comparison is the packed variant with 32-window
batches and 8 copies, selected as plan_create selects it for a plan with enough windows per wavefront (SFS2D_TRI=1
lifts only that condition)."""
import numpy as np
import pytest

import wide_util as U
from oracle import sfs_oracle as O

pytestmark = pytest.mark.gpu

WS = 20000
KNOBS = ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE", "SFS2D_LNL", "SFS2D_LEAN",
         "SFS2D_POOLS", "SFS2D_WGS", "SFS2D_TRI", "SFS2D_SB", "SFS2D_R1", "SFS2D_SLOTS_ONCE")
_DATA = {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    # plan_create packs only plans with >= 8 windows per resident wavefront (tens of thousands of windows); these
    # genomes are small, so the packed variant is asked for whatever that ratio (test_gate_* leaves the rule alone)
    monkeypatch.setenv("SFS2D_TRI", "1")


def _packed(counts, pos, off):
    from sfs2d.pack import PackedSNPs
    counts = np.concatenate(counts).astype(np.uint32)
    return PackedSNPs(counts, np.concatenate(pos).astype(np.uint32), np.array(off, np.int64),
                      [f"chr{c:04d}" for c in range(len(off) - 1)], np.zeros(len(counts), np.uint16),
                      ["intergenic_region"], "p1", "p2")


def _windows(groups):
    """One chromosome's positions: window w holds groups[w] SNPs, evenly spaced inside its 20 kb."""
    return [w * WS + 1 + np.arange(k, dtype=np.int64) * (19000 // k) for w, k in enumerate(groups) if k]


def _run(p, cfg, env=None, monkeypatch=None):
    """One plan of cfg on uploaded data, run once: (records, Fst, scan_variant, scan_packing)."""
    from sfs2d.engine import Engine
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        dev = Engine.get(0).upload(p)
        try:
            pl = dev.eng.plan(dev, cfg)
            try:
                pl.run()
                pl.check()
                return pl.read(), pl.read_fst(), pl.scan_variant(), pl.scan_packing()
            finally:
                pl.close()
        finally:
            dev.close()
    finally:
        for k in env or {}:
            monkeypatch.delenv(k)
        if env and "SFS2D_TRI" in env:
            monkeypatch.setenv("SFS2D_TRI", "1")   # (the fixture's setting)


def _same_bits(a, b):
    assert a[0].tobytes() == b[0].tobytes()   # 64-B records
    assert a[1].tobytes() == b[1].tobytes()   # Fst (NaNs included)
    assert a[2] == b[2]                       # the reported (lean) variant


# ------------------------------------------------------------------------------------------------ packing

def _bins_genome(npop):
    """Chromosome 0: window 0 one SNP in every reachable folded bin (x1 + x2 <= n, n = 2 npop, (0, 0) too), window 1
    two in each (one keyed by its alternative counts, one by its reference counts -- a1 + a2 > n folds), window 2
    the diagonal x1 + x2 = n, window 3 the folding rows x1 > n / 2 with missing calls in both populations (called
    counts below 2 pop_size), window 4 empty, window 5 the rows again keyed by the reference side.  Chromosome 1:
    a synthetic one, five windows."""
    if npop in _DATA:
        return _DATA[npop]
    from sfs2d.pack import pack_counts
    from sfs2d.synth import synth_chrom
    n = 2 * npop
    rng = np.random.Generator(np.random.PCG64(1300 + npop))
    x1, x2 = np.array([(a, b) for a in range(n + 1) for b in range(n + 1 - a)], np.int64).T
    alt = pack_counts(n - x1, x1, n - x2, x2)        # key: the alternative counts (a1 + a2 <= n)
    ref = pack_counts(x1, n - x1, x2, n - x2)        # key: the reference counts (a1 + a2 >= n)
    diag = x1 + x2 == n
    rows = x1 > npop
    m1, m2 = rng.integers(0, n - x1[rows] + 1), rng.integers(0, n - x2[rows] - x1[rows] + 1)   # missing calls
    miss_alt = pack_counts(n - x1[rows] - m1, x1[rows], n - x2[rows] - m2, x2[rows])
    # ... and SNPs with fewer than 2 called alleles in population 1 (Fst drops them: the FST 3 variants)
    low = pack_counts([1, 0, 0], [0, 1, 0], [n - 2, n - 1, n - 3], [2, 1, 3])
    miss_alt = np.concatenate([miss_alt, low])
    # (keyed by the reference side: the alternative counts lose the missing calls and a1 + a2 stays above n)
    r1, r2 = x1[rows], x2[rows]
    m1 = rng.integers(0, np.maximum(1, n - r1 - r2))
    miss_ref = pack_counts(r1, n - r1 - m1, r2, n - r2)[m1 < n - r1 - r2]
    win = [rng.permutation(alt), rng.permutation(np.concatenate([alt, ref])), np.concatenate([alt[diag], ref[diag]]),
           rng.permutation(miss_alt), np.zeros(0, np.uint32), rng.permutation(miss_ref)]
    c0 = np.concatenate(win)
    _, s1, t1, s2, t2 = synth_chrom(rng, 1500, npop, npop)
    p = _packed([c0, pack_counts(s1, t1, s2, t2)], _windows([len(w) for w in win]) + _windows([300] * 5),
                [0, len(c0), len(c0) + 1500])
    _DATA[npop] = p
    return p


@pytest.mark.parametrize("npop,fused", [(3, 1), (3, 0), (12, 1), (12, 0), (25, 1), (25, 0), (31, 1), (31, 0)])
def test_packed_equals_lean(monkeypatch, npop, fused):
    """3/3, 12/12 and 25/25 (n + 1 = 7, 25, 51) run packed.  31/31 cannot: its 63 x 63 lp table, D, F and Fst tables
    take about 39 KB and eight packed u16 histograms with four 1D copies 40,448 B, so even the arm with nothing
    bought needs about 84 KB with its static LDS -- above the 80 KB plan_create allows a packed workgroup.  The case pins that
    fall-back: the lean variant, reported as such, with the lean results."""
    from sfs2d.engine import ScanConfig
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    p = _bins_genome(npop)
    cfg = ScanConfig(n1p=npop, n2p=npop, window=WS, fst=True)
    tri = _run(p, cfg)
    lean = _run(p, cfg, {"SFS2D_TRI": "0"}, monkeypatch)
    assert lean[3] == dict(tri=0, sb=8, r1=4), lean[3]
    assert tri[2] == dict(p16=1, fused=fused, fst=3, cnt=1, gate=1, tri=-1), tri[2]
    # (31/31: the 63 x 63 tables leave no 80 KB workgroup -- plan_create's fall-back, the lean variant again)
    assert tri[3] == (dict(tri=1, sb=32, r1=8) if npop <= 25 else dict(tri=0, sb=8, r1=4)), tri[3]
    _same_bits(tri, lean)
    n = 2 * npop
    recs = tri[0]
    w0 = recs[(recs["chrom"] == 0) & (recs["wid"] == 0)][0]
    assert int(w0["n2"]) == (n + 1) * (n + 2) // 2 - 1   # every reachable bin but (0, 0)
    if npop in (12, 25):   # against the oracle, once per flavour
        wins = O.bp_windows(p, WS)
        ocfg = O.Cfg(npop, npop)
        bg = O.chrom_backgrounds(p, ocfg)
        U.check_against_oracle(recs, tri[1], p, wins, ocfg, lambda c: bg[c], key=("tri-bins", npop))


def _wide_genome():
    """12/12 with a window of 66,000 SNPs at four per position -- every reachable bin in turn, then synthetic ones --
    so that plan_create takes 32-bit 2D bins (p16 = 0) and the window, its size saturated in the record, the exact
    path (eval_exact on packed bins); an ordinary window after it and an ordinary second chromosome."""
    if "wide" in _DATA:
        return _DATA["wide"]
    from sfs2d.pack import pack_counts
    from sfs2d.synth import synth_chrom
    n = 24
    rng = np.random.Generator(np.random.PCG64(1381))
    x1, x2 = np.array([(a, b) for a in range(n + 1) for b in range(n + 1 - a)], np.int64).T
    bins = np.concatenate([pack_counts(n - x1, x1, n - x2, x2), pack_counts(x1, n - x1, x2, n - x2)])
    _, r1, a1, r2, a2 = synth_chrom(rng, 66000 - 40 * len(bins) + 300 + 1500, 12, 12)
    syn = pack_counts(r1, a1, r2, a2)
    k = 66000 - 40 * len(bins)
    big = rng.permutation(np.concatenate([np.tile(bins, 40), syn[:k]]))
    c0 = np.concatenate([big, syn[k:k + 300]])
    pos0 = np.concatenate([1 + np.arange(66000) // 4, WS + 1 + np.arange(300) * 60])
    pos1 = 1 + np.arange(1500) * 60
    p = _packed([c0, syn[k + 300:]], [pos0, pos1], [0, len(c0), len(c0) + 1500])
    _DATA["wide"] = p
    return p


@pytest.mark.parametrize("fused", [1, 0])
def test_packed_32_bit_bins(monkeypatch, fused):
    """The P16 = false instantiations, against the lean variant (which tests/test_position_edges.py pins to the
    oracle at 32-bit bins)."""
    from sfs2d.engine import ScanConfig
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    p = _wide_genome()
    cfg = ScanConfig(n1p=12, n2p=12, window=WS, fst=True)
    tri = _run(p, cfg)
    lean = _run(p, cfg, {"SFS2D_TRI": "0"}, monkeypatch)
    assert tri[2] == dict(p16=0, fused=fused, fst=2, cnt=1, gate=1, tri=-1), tri[2]
    assert tri[3] == dict(tri=1, sb=32, r1=8) and lean[3] == dict(tri=0, sb=8, r1=4), (tri[3], lean[3])
    _same_bits(tri, lean)
    assert int(tri[0]["end"][0]) - int(tri[0]["begin"][0]) == 66000 and int(tri[0]["n2"][0]) > 40000


@pytest.mark.parametrize("knob,value", [("SFS2D_SB", "16"), ("SFS2D_SB", "64"), ("SFS2D_R1", "2"), ("SFS2D_R1", "x")])
def test_unknown_arm_values_are_refused(monkeypatch, knob, value):
    from sfs2d._lib import Sfs2dError
    from sfs2d.engine import ScanConfig
    with pytest.raises(Sfs2dError, match="SFS2D_SB must be 8 or 32"):
        _run(_batch_genome(), ScanConfig(n1p=25, n2p=25, window=WS, fst=True), {knob: value}, monkeypatch)


def test_gate_on_windows_per_wavefront(monkeypatch):
    """plan_create's own rule, SFS2D_TRI unset: a plan with fewer than 8 windows per resident wavefront keeps the
    lean variant; one chromosome of 70,000 window slots (a SNP in every other one: 17 windows per wavefront on
    256 CUs, 2 workgroups of 8 each) runs packed, with the lean results."""
    from sfs2d.engine import ScanConfig
    from sfs2d.pack import pack_counts
    from sfs2d.synth import synth_chrom
    monkeypatch.delenv("SFS2D_TRI")
    cfg = ScanConfig(n1p=25, n2p=25, window=WS, fst=True)
    assert _run(_batch_genome(), cfg)[3] == dict(tri=0, sb=8, r1=4)
    rng = np.random.Generator(np.random.PCG64(1409))
    _, r1, a1, r2, a2 = synth_chrom(rng, 35000, 25, 25)
    p = _packed([pack_counts(r1, a1, r2, a2)], [1 + 2 * WS * np.arange(35000, dtype=np.int64)], [0, 35000])
    packed = _run(p, cfg)
    assert packed[3] == dict(tri=1, sb=32, r1=8), packed[3]
    assert len(packed[0]) >= 69999
    lean = _run(p, cfg, {"SFS2D_TRI": "0"}, monkeypatch)
    assert lean[3] == dict(tri=0, sb=8, r1=4), lean[3]
    _same_bits(packed, lean)


# ------------------------------------------------------------------------------------------------ batches

def _batch_genome():
    """One chromosome of 8 x 33 + 41 = 305 window slots holding 0 to 3 SNPs each (every fourth one empty, a run of
    five empty ones in the middle): with one workgroup its 8 wavefronts take ~38 windows each through the pool
    counters -- a full batch of 32, its boundary, and a partial batch at the end."""
    if "batch" in _DATA:
        return _DATA["batch"]
    from sfs2d.pack import pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(1313))
    groups = [0 if w % 4 == 2 or 150 <= w < 155 else 1 + (w * 7) % 3 for w in range(8 * 33 + 41)]
    groups[-1] = 3
    n = sum(groups)
    _, r1, a1, r2, a2 = synth_chrom(rng, n, 25, 25)
    p = _packed([pack_counts(r1, a1, r2, a2)], _windows(groups), [0, n])
    _DATA["batch"] = p
    return p


@pytest.mark.parametrize("fused", [1, 0])
def test_batches_of_32(monkeypatch, fused):
    from sfs2d.engine import ScanConfig
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    p = _batch_genome()
    cfg = ScanConfig(n1p=25, n2p=25, window=WS, fst=True)
    one = _run(p, cfg, {"SFS2D_WGS": "1"}, monkeypatch)
    assert one[3] == dict(tri=1, sb=32, r1=8), one[3]
    assert len(one[0]) > 8 * 33
    sb8 = _run(p, cfg, {"SFS2D_WGS": "1", "SFS2D_SB": "8"}, monkeypatch)
    assert sb8[3] == dict(tri=1, sb=8, r1=8), sb8[3]
    _same_bits(one, sb8)
    lean = _run(p, cfg, {"SFS2D_WGS": "1", "SFS2D_TRI": "0"}, monkeypatch)
    assert lean[3] == dict(tri=0, sb=8, r1=4), lean[3]
    _same_bits(one, lean)
    _same_bits(one, _run(p, cfg))   # the default grid
    if fused:
        wins = O.bp_windows(p, WS)
        ocfg = O.Cfg(25, 25)
        bg = O.chrom_backgrounds(p, ocfg)
        U.check_against_oracle(one[0], one[1], p, wins, ocfg, lambda c: bg[c], key=("tri-batch",))


# ------------------------------------------------------------------------------------------------ lane copies

def _copies_genome():
    """Windows of 600 SNPs in one folded 1D bin of each population -- bin 0, bin 1, bin n_p -- then one of 1,100 SNPs
    with 600 in one 2D bin of a folding row (x1 = 30 > n / 2: its packed place is not its key) and 500 synthetic
    ones: the streamed rows, the sweep clear and the over-LNT correction on packed bins.  A synthetic window
    last."""
    if "copies" in _DATA:
        return _DATA["copies"]
    from sfs2d.pack import pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(1327))
    n = 50
    one = lambda a1, a2, k: np.full(k, int(pack_counts([n - a1], [a1], [n - a2], [a2])[0]), np.uint32)
    _, r1, a1, r2, a2 = synth_chrom(rng, 900, 25, 25)
    syn = pack_counts(r1, a1, r2, a2)
    big = rng.permutation(np.concatenate([one(30, 7, 600), syn[:500]]))
    win = [one(0, 0, 600), one(1, 1, 600), one(25, 25, 600), big, syn[500:]]
    c = np.concatenate(win)
    p = _packed([c], _windows([len(w) for w in win]), [0, len(c)])
    _DATA["copies"] = p
    return p


@pytest.mark.parametrize("fused", [1, 0])
def test_eight_lane_copies(monkeypatch, fused):
    from sfs2d.engine import ScanConfig
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    p = _copies_genome()
    cfg = ScanConfig(n1p=25, n2p=25, window=WS, fst=True)
    r8 = _run(p, cfg)
    assert r8[3] == dict(tri=1, sb=32, r1=8), r8[3]
    r4 = _run(p, cfg, {"SFS2D_R1": "4"}, monkeypatch)
    assert r4[3] == dict(tri=1, sb=32, r1=4), r4[3]
    _same_bits(r8, r4)
    _same_bits(r8, _run(p, cfg, {"SFS2D_TRI": "0"}, monkeypatch))
    recs = r8[0]
    assert [int(x) for x in recs["snp_count"][:4]] == [600, 600, 600, 1100]
    assert [int(x) for x in recs["n1a"][:3]] == [0, 600, 0] and int(recs["n2"][3]) >= 600
    if fused:
        wins = O.bp_windows(p, WS)
        ocfg = O.Cfg(25, 25)
        bg = O.chrom_backgrounds(p, ocfg)
        U.check_against_oracle(recs, r8[1], p, wins, ocfg, lambda c: bg[c], key=("tri-copies",))


# ------------------------------------------------------------------------------------------------ ineligible plans

@pytest.mark.parametrize("name", ["overcalled", "unfolded", "n1_ne_n2"])
def test_ineligible_plans_keep_their_variant(monkeypatch, name):
    from sfs2d.engine import ScanConfig
    from sfs2d.pack import pack_counts
    p = _bins_genome(25)
    cfg = ScanConfig(n1p=25, n2p=25, window=WS, fst=True)
    want = dict(p16=1, fused=1, fst=3, cnt=1, gate=1, tri=-1)
    if name == "overcalled":   # nc_ok false: one SNP called above 2 pop_size keeps the range test (gate 0)
        c = p.counts.copy()
        c[5] = int(pack_counts([40], [20], [30], [10])[0])
        p = _packed([c], [p.pos], list(p.chrom_off))
        want["gate"] = 0
    elif name == "unfolded":
        cfg = ScanConfig(n1p=25, n2p=25, fold=False, window=WS, fst=True)
        want["gate"] = 0
    else:   # 25/20 on the 25/25 counts would be over-called: a genome of its own
        from sfs2d.synth import synth_chrom
        rng = np.random.Generator(np.random.PCG64(1361))
        _, r1, a1, r2, a2 = synth_chrom(rng, 1500, 25, 20)
        p = _packed([pack_counts(r1, a1, r2, a2)], _windows([300] * 5), [0, 1500])
        cfg = ScanConfig(n1p=25, n2p=20, window=WS, fst=True)
        want["fst"] = 3 if bool(np.any((r1 + a1 < 2) | (r2 + a2 < 2))) else 2
    monkeypatch.setenv("SFS2D_FUSED", "1")
    a = _run(p, cfg)
    b = _run(p, cfg, {"SFS2D_TRI": "0"}, monkeypatch)
    assert a[2] == want, (a[2], want)
    assert a[3] == dict(tri=0, sb=8, r1=4) and b[3] == a[3], (a[3], b[3])
    _same_bits(a, b)


# ------------------------------------------------------------------------------------------------ the benchmarked shape

def test_benchmarked_shape(monkeypatch):
    """The headline loop in small: per-chromosome backgrounds at 25/25, 20 kb windows of ~360 SNPs, Fst, the scan
    capped at one workgroup per CU, two plans on two streams through Plan.run_streams."""
    import torch
    from sfs2d.engine import Engine, Plan, ScanConfig
    from sfs2d.pack import pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(1399))
    counts, pos, off = [], [], [0]
    for _ in range(4):
        ps, r1, a1, r2, a2 = synth_chrom(rng, 20000, 25, 25, mean_gap=56.0)
        counts.append(pack_counts(r1, a1, r2, a2))
        pos.append(ps)
        off.append(off[-1] + 20000)
    p = _packed(counts, pos, off)
    cfg = ScanConfig(n1p=25, n2p=25, window=WS, fst=True, scan_wgs_per_cu=1)
    eng = Engine.get(0)
    dev = eng.upload(p)
    try:
        ref = eng.plan(dev, cfg)
        try:
            ref.run()
            ref.check()
            want, want_fst, packing = ref.read(), ref.read_fst(), ref.scan_packing()
        finally:
            ref.close()
        assert packing == dict(tri=1, sb=32, r1=8), packing
        streams = [torch.cuda.Stream(device=torch.device("cuda:0")) for _ in range(2)]
        plans = [eng.plan(dev, cfg) for _ in range(2)]
        try:
            outs = [torch.zeros(pl.nrec * 64, dtype=torch.uint8, device="cuda:0") for pl in plans]
            torch.cuda.synchronize()
            Plan.run_streams(plans, [s.cuda_stream for s in streams], 5, [o.data_ptr() for o in outs])
            for s in streams:
                s.synchronize()
            for k, pl in enumerate(plans):
                pl.check()
                assert outs[k].cpu().numpy().tobytes() == want.tobytes(), k
                assert pl.read_fst().tobytes() == want_fst.tobytes(), k
        finally:
            for pl in plans:
                pl.close()
    finally:
        dev.close()
    # 50 windows against the oracle
    from sfs2d import _lib as L
    wins = O.bp_windows(p, WS)
    live = (want["flags"] & (L.W_EMPTY | L.W_EXTRA)) == 0
    body, fl = want[live], want_fst[: len(live)][live]
    assert len(body) == len(wins) and len(wins) >= 200
    idx = np.sort(rng.choice(len(wins), 50, replace=False))
    ocfg = O.Cfg(25, 25)
    bg = O.chrom_backgrounds(p, ocfg)
    refo = U.oracle_ref(p, [wins[i] for i in idx], ocfg, lambda c: bg[c])
    U.check_records(body[idx], fl[idx], refo)
