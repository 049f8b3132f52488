"""Window slots from the data set's position index (k_pos_index / k_slots_index): fixed-bp counts plans with
per-chromosome backgrounds take their slot table from the index, ahead of a k_prep that reads no positions
(SFS2D_SEG=index, the default for them), instead of k_prep's segmentation pass (SFS2D_SEG=prep).  The two
write the same table -- (first + 1, last + 1), (0, 0) for an empty window, every slot on every run -- so the
records are compared as bytes and Fst as bits."""
import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

LENGTHS = [5000, 1, 3000, 70, 900]
ENV = ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE", "SFS2D_WGS", "SFS2D_LNL", "SFS2D_LEAN",
       "SFS2D_JNT")
_DATA = {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _genome(n):
    """Windows of a few SNPs (3 kb) and of one, a one-SNP chromosome, two k_prep tiles in chromosome 0 (empty
    windows: _edges)."""
    if ("g", n) not in _DATA:
        from sfs2d.synth import synth_genome
        _DATA["g", n] = synth_genome(5, LENGTHS, n, n, seed=1000 + n)
    return _DATA["g", n]


def _edges(n):
    """Hand-built positions (every window size below divides 500,000 and 3,000,000):
    chromosome 0 -- position 0, duplicates on the boundary values j ws and j ws + 1 (1,000 / 1,001 and 500,000 /
      500,001), a gap from 600,000 to 2,500,000 (many empty cells and windows), last position 3,000,000 =
      a multiple of every ws; its cells are 32,768 bp: a 100 bp window is far smaller, a 500 kb one far larger;
    chromosome 1 -- 200 SNPs within 100 bp at 1,000,000 (duplicates): all in the index's last cell;
    chromosome 2 -- 20 SNPs: an index of one cell;
    chromosome 3 -- one SNP at position 0."""
    if ("e", n) in _DATA:
        return _DATA["e", n]
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(77 + n))
    special = [0, 1, 1000, 1000, 1001, 1001, 500000, 500000, 500001, 500001, 3000000]
    c0 = np.sort(np.concatenate([special, rng.integers(2, 600000, size=1500), rng.integers(2500000, 3000000, size=500)]))
    c1 = np.sort(rng.integers(1000000, 1000101, size=200))
    c2 = np.sort(rng.integers(100000, 100500, size=20))
    pos = [c0, c1, c2, np.array([0])]
    counts = []
    for x in pos:
        _, r1, a1, r2, a2 = synth_chrom(rng, len(x), n, n)
        counts.append(pack_counts(r1, a1, r2, a2))
    off = np.concatenate([[0], np.cumsum([len(x) for x in pos])]).astype(np.int64)
    nsnp = int(off[-1])
    p = PackedSNPs(np.concatenate(counts), np.concatenate(pos).astype(np.uint32), off, [f"chr{i:04d}" for i in range(4)],
                   np.zeros(nsnp, np.uint16), ["intergenic_region"], "p1", "p2")
    _DATA["e", n] = p
    return p


def _cfg(n, ws, fst, **kw):
    from sfs2d import _lib as L
    from sfs2d.engine import ScanConfig
    return ScanConfig(n1p=n, n2p=n, window=ws, bg_mode=L.BG_PER_CHROM, fst=fst, **kw)


def _scan(monkeypatch, eng, dev, cfg, flag, kernel):
    """Records and Fst of a plan created under SFS2D_SEG=flag and run twice."""
    monkeypatch.setenv("SFS2D_SEG", flag)
    pl = eng.plan(dev, cfg)
    try:
        kind = pl.seg_kind()
        assert pl.scan_kernel() == kernel
        for _ in range(2):   # every slot is rewritten on every run
            pl.run()
            pl.check()
        return kind, pl.read(), (pl.read_fst() if cfg.fst else np.zeros(0))
    finally:
        pl.close()


def _index_equals_prep(monkeypatch, p, n, ws):
    from sfs2d.engine import Engine
    eng = Engine.get(0)
    dev = eng.upload(p)
    kernel = "k_scan_w" if n == 25 else "k_scan_gw"
    try:
        for fst in (False, True):
            cfg = _cfg(n, ws, fst)
            ki, ri, fi = _scan(monkeypatch, eng, dev, cfg, "index", kernel)
            kp, rp, fp = _scan(monkeypatch, eng, dev, cfg, "prep", kernel)
            # (k_scan_gw plans with Fst keep k_prep's Fst sums, and with them its segmentation)
            assert ki == ("prep" if (fst and n == 50) else "index") and kp == "prep", (ki, kp)
            assert len(ri) == len(rp) and ri.tobytes() == rp.tobytes()
            assert fi.tobytes() == fp.tobytes()
    finally:
        dev.close()


@pytest.mark.parametrize("n", [25, 50])
@pytest.mark.parametrize("ws", [3000, 20000, 65535])
def test_index_equals_segmentation(monkeypatch, ws, n):
    _index_equals_prep(monkeypatch, _genome(n), n, ws)


@pytest.mark.parametrize("n", [25, 50])
@pytest.mark.parametrize("ws", [100, 1000, 500000])
def test_index_equals_segmentation_edges(monkeypatch, ws, n):
    _index_equals_prep(monkeypatch, _edges(n), n, ws)


def test_lean_variant_runs_on_index_slots(monkeypatch):
    """n = 25 with Fst is the headline class: k_scan_w's LEAN variant (gated, Fst in the scan) behind a
    histogram-only k_prep."""
    from sfs2d.engine import Engine
    eng = Engine.get(0)
    dev = eng.upload(_genome(25))
    pl = eng.plan(dev, _cfg(25, 20000, True))
    try:
        assert pl.seg_kind() == "index"
        pl.run()
        pl.check()
        v = pl.scan_variant()
        assert v["gate"] == 1 and v["cnt"] == 1 and v["fst"] in (2, 3)
    finally:
        pl.close()
        dev.close()


def test_wrapped_device_arrays_keep_segmentation(monkeypatch):
    """The contents of wrapped device arrays are the caller's (they may be written after the plan is created,
    tests/test_stream_contract.py): no index is built from them, the plan segments in k_prep -- same records."""
    import torch
    from sfs2d.engine import Engine
    n = 25
    p = _genome(n)
    eng = Engine.get(0)
    dev = eng.upload(p)
    cfg = _cfg(n, 20000, True)
    try:
        kind, want, want_f = _scan(monkeypatch, eng, dev, cfg, "index", "k_scan_w")
    finally:
        dev.close()
    assert kind == "index"
    counts = torch.zeros(p.n + 64, dtype=torch.int32, device="cuda:0")
    pos = torch.zeros(p.n + 64, dtype=torch.int32, device="cuda:0")
    counts[:p.n].copy_(torch.from_numpy(p.counts.view(np.int32)))
    pos[:p.n].copy_(torch.from_numpy(p.pos.view(np.int32)))
    torch.cuda.synchronize()
    d = eng.wrap_device(counts.data_ptr(), pos.data_ptr(), None, p.n, p.chrom_off, p.pos[p.chrom_off[1:] - 1])
    try:
        kind, got, got_f = _scan(monkeypatch, eng, d, cfg, "index", "k_scan_w")
    finally:
        d.close()
    assert kind == "prep"
    assert got.tobytes() == want.tobytes() and got_f.tobytes() == want_f.tobytes()


def test_index_outlives_plans(monkeypatch):
    """The index belongs to the data set: plans of three window sizes in turn over one data set, the first
    closed before the last is created."""
    from sfs2d.engine import Engine
    n = 25
    p = _genome(n)
    eng = Engine.get(0)
    dev = eng.upload(p)
    sizes = (3000, 20000, 65535)
    try:
        want = [_scan(monkeypatch, eng, dev, _cfg(n, ws, True), "prep", "k_scan_w") for ws in sizes]
        monkeypatch.setenv("SFS2D_SEG", "index")
        a = eng.plan(dev, _cfg(n, sizes[0], True))
        a.run()
        a.check()
        got = [(a.seg_kind(), a.read(), a.read_fst())]
        b = eng.plan(dev, _cfg(n, sizes[1], True))
        a.close()
        c = eng.plan(dev, _cfg(n, sizes[2], True))
        for q in (b, c):
            q.run()
            q.check()
            got.append((q.seg_kind(), q.read(), q.read_fst()))
            q.close()
        for (k, r, f), (_, wr, wf) in zip(got, want):
            assert k == "index"
            assert r.tobytes() == wr.tobytes() and f.tobytes() == wf.tobytes()
    finally:
        dev.close()


def test_streams_and_graph(monkeypatch):
    """The benchmark's plan shape at small size: scan_wgs_per_cu = 1, the joint-histogram k_prep, two plans
    round-robin on two streams (sfs2d_plan_run_streams, staggered start), several runs, then one graph replay:
    each plan writes what a segmenting plan writes run alone."""
    import torch
    from sfs2d.engine import Engine, Plan
    n = 25
    p = _genome(n)
    monkeypatch.setenv("SFS2D_JNT", "1")
    eng = Engine.get(0)
    dev = eng.upload(p)
    cfg = _cfg(n, 20000, True, scan_wgs_per_cu=1)
    _, want, want_f = _scan(monkeypatch, eng, dev, cfg, "prep", "k_scan_w")
    monkeypatch.setenv("SFS2D_SEG", "index")
    plans = [eng.plan(dev, cfg) for _ in range(2)]
    assert all(q.seg_kind() == "index" for q in plans)
    streams = [torch.cuda.Stream(device=0).cuda_stream for _ in range(2)]
    outs = [torch.zeros((plans[0].nrec, 64), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    optrs = [o.data_ptr() for o in outs]

    def check_all():
        torch.cuda.synchronize()
        for k, q in enumerate(plans):
            q.check()
            assert outs[k].cpu().numpy().tobytes() == want.tobytes()
            assert q.read_fst().tobytes() == want_f.tobytes()

    try:
        Plan.run_streams(plans, streams, 6, optrs)
        check_all()
        g = Plan.graph(plans, streams, 4, optrs)
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        g.launch(1)
        check_all()
        g.close()
    finally:
        for q in plans:
            q.close()
        dev.close()


def test_index_vs_oracle(monkeypatch):
    """The index path against the oracle's window_records (per-chromosome backgrounds, 3 kb windows)."""
    from oracle import sfs_oracle as O
    from sfs2d import _lib as L
    from sfs2d.engine import Engine
    n, ws = 25, 3000
    p = _genome(n)
    eng = Engine.get(0)
    dev = eng.upload(p)
    try:
        kind, recs, _ = _scan(monkeypatch, eng, dev, _cfg(n, ws, False), "index", "k_scan_w")
    finally:
        dev.close()
    assert kind == "index"
    cfg_o = O.Cfg(n, n)
    bgs = O.chrom_backgrounds(p, cfg_o)
    ref = O.window_records(p, O.bp_windows(p, ws), cfg_o, lambda c: bgs[c])
    body = recs[(recs["flags"] & L.W_EMPTY) == 0]
    assert len(body) == len(ref)
    for r, o in zip(body, ref):
        assert int(r["snp_count"]) == o["snp_count"] and int(r["n2"]) == o["N2"]
        for f, g in (("t2d", "T2D"), ("t1d_p1", "T1D_p1"), ("t1d_p2", "T1D_p2")):
            if o[g] is not None:
                assert gu.close(float(r[f]), o[g]), (f, float(r[f]), o[g])
