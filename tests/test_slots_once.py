"""The slot table written once per plan: "index" plans whose scan sums Fst itself never store to their slot table,
and the table depends on the data set's position index, the window and the slot bases alone, so only the plan's
first run launches k_slots_index (sfs2d_plan_slots_once = 1; SFS2D_SLOTS_ONCE=0 at plan creation: every run).

Three chromosomes of a few thousand SNPs, 25/25, 20 kb windows with Fst.  Every run of a plan writes the same
table, so after 1, 2 and 5 runs -- plain, split into phases, through run_streams, replayed from a graph -- the
records and the Fst column must equal, as bytes, those of a plan created with SFS2D_SLOTS_ONCE=0 and run once;
that table is compared with the oracle as in test_scan_variants.py.  A run that skipped the slot kernel before
the table was there would scan empty slots.  Plans outside the class report 0 and keep their per-run table."""
import numpy as np
import pytest

import wide_util as U
from oracle import sfs_oracle as O

pytestmark = pytest.mark.gpu

WS = 20000
_P, _REF = {}, {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE", "SFS2D_LEAN", "SFS2D_WGS",
              "SFS2D_POOLS", "SFS2D_SLOTS_ONCE"):
        monkeypatch.delenv(k, raising=False)


def _genome():
    if "p" not in _P:
        from sfs2d.synth import synth_genome
        _P["p"] = synth_genome(3, [4000, 2500, 3000], 25, 25, seed=11)
    return _P["p"]


def _cfg(window=WS, fst=True):
    from sfs2d.engine import ScanConfig
    return ScanConfig(n1p=25, n2p=25, window=window, fst=fst)


def _table(pl, fst=True):
    pl.check()
    return pl.read().tobytes(), pl.read_fst().tobytes() if fst else b""


def _ref(monkeypatch, dev, fused, window=WS):
    """The table of a plan that writes its slots in every run (SFS2D_SLOTS_ONCE=0), run once."""
    key = (fused, window)
    if key not in _REF:
        monkeypatch.setenv("SFS2D_SLOTS_ONCE", "0")
        pl = dev.eng.plan(dev, _cfg(window))
        monkeypatch.delenv("SFS2D_SLOTS_ONCE")
        try:
            assert pl.seg_kind() == "index" and not pl.slots_once()
            pl.run()
            _REF[key] = _table(pl)
        finally:
            pl.close()
    return _REF[key]


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "sliced"])
def test_repeated_runs_equal_the_per_run_table_and_the_oracle(monkeypatch, fused):
    from sfs2d import _lib as L
    from sfs2d.engine import Engine
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    p = _genome()
    dev = Engine.get(0).upload(p)
    try:
        want = _ref(monkeypatch, dev, fused)
        pl = dev.eng.plan(dev, _cfg())
        try:
            assert pl.seg_kind() == "index" and pl.slots_once()
            for more in (1, 1, 3):   # after 1, 2 and 5 runs
                pl.run_many(more)
                assert _table(pl) == want
            pl.run(phase=1)          # a run split into its stage and its scan
            pl.run(phase=2)
            assert _table(pl) == want
            assert pl.scan_variant()["fused"] == fused
            recs, f = pl.read(), pl.read_fst()
        finally:
            pl.close()
        assert np.any((recs["flags"] & L.W_EMPTY) == 0)
        ocfg = O.Cfg(25, 25)
        bgs = O.chrom_backgrounds(p, ocfg)
        U.check_against_oracle(recs, f, p, O.bp_windows(p, WS), ocfg, lambda c: bgs[c], key=("slots_once", WS))
    finally:
        dev.close()


def test_run_streams_and_graph_replay(monkeypatch):
    import torch
    from sfs2d.engine import Engine, Plan
    monkeypatch.setenv("SFS2D_FUSED", "1")
    eng = Engine.get(0)
    dev = eng.upload(_genome())
    try:
        want = [_ref(monkeypatch, dev, 1, w) for w in (WS, 10000)]
        streams = [torch.cuda.Stream(device=torch.device("cuda:0")) for _ in range(2)]
        sh = [s.cuda_stream for s in streams]
        plans = [eng.plan(dev, _cfg(w)) for w in (WS, 10000)]
        try:
            assert all(pl.slots_once() for pl in plans)
            outs = [torch.zeros(pl.nrec * 64, dtype=torch.uint8, device="cuda:0") for pl in plans]
            torch.cuda.synchronize()
            # captured before the plans have run: the tables are written ahead of the capture, not by a replay
            g = Plan.graph(plans, sh, 4, [o.data_ptr() for o in outs])
            try:
                Plan.run_streams(plans, sh, 5, [o.data_ptr() for o in outs])   # plan 0 three times, plan 1 twice
                for s in streams:
                    s.synchronize()
                for k in range(2):
                    assert outs[k].cpu().numpy().tobytes() == want[k][0], k
                    assert plans[k].read_fst().tobytes() == want[k][1], k
                plans[0].run(outs[0].data_ptr())   # (an even number of runs of every plan before the replay)
                for o in outs:
                    o.zero_()
                torch.cuda.synchronize()
                g.launch(2)
                for s in streams:
                    s.synchronize()
                for k in range(2):
                    plans[k].check()
                    assert outs[k].cpu().numpy().tobytes() == want[k][0], k
                    assert plans[k].read_fst().tobytes() == want[k][1], k
            finally:
                g.close()
        finally:
            for pl in plans:
                pl.close()
    finally:
        dev.close()


def test_stage_timing_rides_in_k_prep(monkeypatch):
    """Sampled runs after the first carry the stage's start event in k_prep's packet: both kernels still time."""
    from sfs2d.engine import Engine
    monkeypatch.setenv("SFS2D_FUSED", "1")
    dev = Engine.get(0).upload(_genome())
    try:
        want = _ref(monkeypatch, dev, 1)
        pl = dev.eng.plan(dev, _cfg())
        try:
            pl.set_timing(3, kernels=5)
            pl.run_many(3)
            n, (k1, _, k3) = pl.timing_read()
            assert n == 3 and 0.0 < k1 < 50.0 and 0.0 < k3 < 50.0, (n, k1, k3)
            pl.set_timing(0)
            assert _table(pl) == want
        finally:
            pl.close()
    finally:
        dev.close()


@pytest.mark.parametrize("name", ["fst_free", "wrapped", "seg_prep"])
def test_plans_outside_the_class_write_their_table_in_every_run(monkeypatch, name):
    from sfs2d.engine import Engine
    monkeypatch.setenv("SFS2D_FUSED", "1")
    eng = Engine.get(0)
    keep = None
    if name == "wrapped":
        dev, keep = U.wrapped(eng, _genome())
    else:
        dev = eng.upload(_genome())
    if name == "seg_prep":
        monkeypatch.setenv("SFS2D_SEG", "prep")
    try:
        fst = name != "fst_free"   # (without Fst the scan clears every slot record it has read)
        pl = eng.plan(dev, _cfg(fst=fst))
        try:
            assert not pl.slots_once()
            assert pl.seg_kind() == ("index" if name == "fst_free" else "prep")
            pl.run()
            first = _table(pl, fst)
            pl.run_many(3)
            assert _table(pl, fst) == first
        finally:
            pl.close()
        if name == "seg_prep":   # k_prep's segmentation of the same upload: the index plans' table
            monkeypatch.delenv("SFS2D_SEG", raising=False)
            up = eng.upload(_genome())
            try:
                assert first == _ref(monkeypatch, up, 1)
            finally:
                up.close()
    finally:
        dev.close()
        del keep
