"""k_scan_w's LEAN variants (gated Fst-in-scan plans with fixed-bp slot records and n1p, n2p <= 31: the window
loop's tail compiled for that class) against the gated variants they replace and against the oracle.

One synthetic chromosome set: 20 kb windows holding 0, 1, 63, 64, 65, 128, 129, 384, 385, 512, 513 and 1,100 SNPs
in turn (no row, one partial row, a full row and one SNP more, one pair, the first 8 rows exactly and the streamed
rows past them, the D table's clamp), on chromosomes of 8, 16, 56, 64, 72, 128 and 136 slots.  SFS2D_WGS=1 gives
every chromosome one workgroup of 8 wavefronts, which share its slots through the pool counters: about 1, 2, 7,
8, 9, 16 and 17 windows per wavefront -- batches of 8 that end early, exactly and one window later, empty slots
at every place in them.

Each plan of the class runs twice, SFS2D_LEAN unset and SFS2D_LEAN=0 (the gated variant): the record tables must
be equal as bytes and the Fst columns as bits; the lean run is then compared with the oracle as in
test_scan_variants.py (integers exact, T by golden_util.close, Fst within 1e-12 + 1e-10 |x|).  Plans outside the
class (n1p = 32, SNP-count windows, a variant_type filter, over-called data) must give the same table with and
without SFS2D_LEAN=0 and match the oracle too.  sfs2d_plan_scan_variant reports a lean plan as its gated
variant (gate = 1; the ABI has no seventh output), so `_in_class` restates plan_create's rule from the reported
variant and the configuration."""
import numpy as np
import pytest

import wide_util as U
from oracle import sfs_oracle as O

pytestmark = pytest.mark.gpu

WS = 20000
SIZES = (0, 1, 63, 64, 65, 128, 129, 384, 385, 512, 513, 1100)
SLOTS = (8, 16, 56, 64, 72, 128, 136)
SMALL = (8, 16, 56)
_DATA, _BG = {}, {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE", "SFS2D_LNL", "SFS2D_LEAN",
              "SFS2D_POOLS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SFS2D_WGS", "1")


def _genome(kind, n1p, n2p, slots):
    """Chromosome c: slots[c] windows of SIZES in turn (starting at a different size per chromosome; a last
    window of 0 SNPs holds 2, the chromosome ends there).  kind "lownc": every 37th SNP has fewer than 2 called
    alleles in a population; "over": three SNPs called above 2 pop_size, one folding to the last bin."""
    key = (kind, n1p, n2p, slots)
    if key in _DATA:
        return _DATA[key]
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(77 + 100 * n1p + n2p))
    counts, pos, off = [], [], [0]
    for c, ns in enumerate(slots):
        sizes = [SIZES[(3 * c + w) % len(SIZES)] for w in range(ns)]
        if sizes[-1] == 0:
            sizes[-1] = 2
        n = sum(sizes)
        _, r1, a1, r2, a2 = synth_chrom(rng, n, n1p, n2p)
        counts.append(pack_counts(r1, a1, r2, a2))
        for w, k in enumerate(sizes):
            if k:
                pos.append(w * WS + 1 + np.arange(k, dtype=np.int64) * (19000 // k))
        off.append(off[-1] + n)
    counts, pos = np.concatenate(counts).astype(np.uint32), np.concatenate(pos).astype(np.uint32)
    pc = lambda r1, a1, r2, a2: int(pack_counts(np.array([r1]), np.array([a1]), np.array([r2]), np.array([a2]))[0])
    if kind == "lownc":
        low = [pc(1, 0, n2p, n2p), pc(0, 1, n2p, n2p), pc(n1p, n1p, 0, 1), pc(0, 0, n2p, n2p), pc(n1p, n1p, 0, 0),
               pc(0, 1, 0, 1)]
        for i, k in enumerate(range(5, len(counts), 37)):
            counts[k] = low[i % len(low)]
    elif kind == "over":
        counts[3] = pc(2 * n1p, n1p + 1, 2 * n2p, n2p)   # folds to (n1, n2), the excluded last bin
        counts[700] = pc(2 * n1p - 10, n1p - 5, n2p + 5, 10)
        counts[off[1] + 9] = pc(n1p + 5, 2 * n1p - 5, n2p - 5, 2 * n2p - 10)
    else:
        assert kind == "plain"
    ann = (np.arange(len(counts)) % 3).astype(np.uint16)
    p = PackedSNPs(counts, pos, np.array(off, np.int64), [f"chr{c:04d}" for c in range(len(slots))], ann,
                   ["intergenic_region", "intron_variant", "missense_variant"], "p1", "p2")
    _DATA[key] = p
    return p


def _bg_of(key, p, ocfg):
    if key not in _BG:
        _BG[key] = O.chrom_backgrounds(p, ocfg)
    return lambda c: _BG[key][c]


def _run(p, cfg):
    """One plan of cfg on uploaded data, run once: (records, Fst, scan_variant, scan kernel)."""
    from sfs2d.engine import Engine
    dev = Engine.get(0).upload(p)
    try:
        pl = dev.eng.plan(dev, cfg)
        try:
            pl.run()
            pl.check()
            return pl.read(), pl.read_fst(), pl.scan_variant(), pl.scan_kernel()
        finally:
            pl.close()
    finally:
        dev.close()


def _in_class(cfg, v, kernel):
    """plan_create's rule for the LEAN variants, from what the plan reports and its configuration."""
    from sfs2d import _lib as L
    return (kernel == "k_scan_w" and v["cnt"] == 1 and v["gate"] == 1 and v["fst"] in (2, 3)
            and cfg.window_mode == L.WINDOW_BP and cfg.ann_want < 0 and cfg.n1p <= 31 and cfg.n2p <= 31)


def _same_bits(a, b):
    assert a[0].tobytes() == b[0].tobytes()   # 64-B records
    assert a[1].tobytes() == b[1].tobytes()   # Fst (NaNs included)
    assert a[2] == b[2] and a[3] == b[3]


def _both(monkeypatch, p, cfg):
    """cfg's plan with SFS2D_LEAN unset and with SFS2D_LEAN=0: equal tables; returns the first run."""
    lean = _run(p, cfg)
    monkeypatch.setenv("SFS2D_LEAN", "0")
    gated = _run(p, cfg)
    monkeypatch.delenv("SFS2D_LEAN")
    _same_bits(lean, gated)
    return lean


LEAN_CASES = [("plain", 25, 25, SLOTS, 2, 1), ("plain", 25, 25, SLOTS, 2, 0), ("lownc", 25, 25, SLOTS, 3, 1),
              ("lownc", 25, 25, SLOTS, 3, 0), ("plain", 31, 10, SMALL, 2, 1)]


@pytest.mark.parametrize("kind,n1p,n2p,slots,fst,fused", LEAN_CASES,
                         ids=[f"{k}-{a}x{b}-fst{f}-{'fused' if u else 'sliced'}" for k, a, b, _, f, u in LEAN_CASES])
def test_lean_equals_gated_and_oracle(monkeypatch, kind, n1p, n2p, slots, fst, fused):
    from sfs2d.engine import ScanConfig
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    p = _genome(kind, n1p, n2p, slots)
    cfg = ScanConfig(n1p=n1p, n2p=n2p, window=WS, fst=True)
    recs, f, v, kernel = _both(monkeypatch, p, cfg)
    assert v == dict(p16=1, fused=fused, fst=fst, cnt=1, gate=1, tri=-1), v
    assert _in_class(cfg, v, kernel)
    wins = O.bp_windows(p, WS)
    assert set(SIZES) - {0} <= {w[3] - w[2] for w in wins}
    assert len(recs) > len(wins)   # empty slots in between
    ocfg = O.Cfg(n1p, n2p)
    key = (kind, n1p, n2p, slots)
    U.check_against_oracle(recs, f, p, wins, ocfg, _bg_of(key, p, ocfg), key=key)


def _outside(name):
    """(data, ScanConfig, oracle Cfg, windows, the variant's gate) of a plan outside the class."""
    from sfs2d import _lib as L
    from sfs2d.engine import ScanConfig
    if name == "n1p32":
        p = _genome("plain", 32, 25, SMALL)
        return p, ScanConfig(n1p=32, n2p=25, window=WS, fst=True), O.Cfg(32, 25), O.bp_windows(p, WS), 1
    if name == "snp500":
        p = _genome("plain", 25, 25, SMALL)
        cfg = ScanConfig(n1p=25, n2p=25, window_mode=L.WINDOW_SNPS, window=500, fst=True)
        return p, cfg, O.Cfg(25, 25), O.snp_windows(p, 500)[0], 1
    if name == "variant_type":
        p = _genome("plain", 25, 25, SMALL)
        cfg = ScanConfig(n1p=25, n2p=25, window=WS, fst=True, ann_want=p.ann_names.index("intron_variant"))
        return p, cfg, O.Cfg(25, 25, "intron_variant"), O.bp_windows(p, WS), 0
    assert name == "overcalled"
    p = _genome("over", 25, 25, SMALL)
    return p, ScanConfig(n1p=25, n2p=25, window=WS, fst=True), O.Cfg(25, 25), O.bp_windows(p, WS), 0


@pytest.mark.parametrize("name", ["n1p32", "snp500", "variant_type", "overcalled"])
def test_plans_outside_the_class_keep_their_variant(monkeypatch, name):
    p, cfg, ocfg, wins, gate = _outside(name)
    recs, f, v, kernel = _both(monkeypatch, p, cfg)   # SFS2D_LEAN has nothing to switch
    assert kernel == "k_scan_w" and v["gate"] == gate, v
    assert not _in_class(cfg, v, kernel)
    key = ("outside", name)
    U.check_against_oracle(recs, f, p, wins, ocfg, _bg_of(key, p, ocfg), key=key)
