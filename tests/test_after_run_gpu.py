"""The post-scan calls after every way of making a plan's last run (include/sfs2d.h: "the plan's last run").

sfs2d_plan_null_run / _null_run_blocks, _diversity, _spectra, _project, _read and _fst_read follow host-side
bookkeeping of the last run: where its records went, the parity of its replica and inner-sum buffers, and whether the
null's background tables were already completed for it.  The other GPU tests make that run by ``run()`` alone.  Here a
SUBJECT plan over one wrapped data set (sfs2d_data_wrap_device) runs once on data set A, the arrays are rewritten to
B (tests/after_util.py: the same host-side facts, other windows and backgrounds), and the last run is made by

  1  run(out_dev_ptr)                      the records in the caller's buffer, the plan's own still A's
  2  run_many                              2 runs into a caller's buffer, then 3 into the plan's: both parities
  3  Plan.run_streams                      two plans, 3 and 4 runs, on the engine's stream and on two torch streams
  4  Plan.graph / RunGraph.launch          two plans on two streams, replayed after each rewrite and once without
  5  run(phase=1), run(out, phase=2)       with no exchange, with the rows doubled, with another data set's rows
  6  Plan.time                             sfs2d_plan_time's own launch sequence

(a) after each of them every array the calls give is byte-equal to a CONTROL's: a plan of the same ScanConfig over an
    upload of the data the arrays hold, after ``run(); check()``;
(b) once per (data set, plan kind) the control itself is held against the twins of the calls' own tests, at their
    tolerances: null_util.check (integers exact, T by golden_util.close with floor 1e-2), div_util.assert_records,
    spectra_util.assert_rows (exact), project_util.assert_grids; its records' integer fields against the oracle's.

A plan that was captured and never executed has no last run: every call refuses it until its graph is launched."""
import numpy as np
import pytest

import after_util as AU
import div_util as DU
import golden_util as gu
import null_util as NU
import project_util as PU
import spectra_util as SU
import split_util as SPL
from sfs2d import _lib as L
from sfs2d import null as N

pytestmark = pytest.mark.gpu

_CONTROL, _ROWS = {}, {}
REC_INTS = ("chrom", "begin", "end", "snp_count", "n2", "n2_all", "n1a", "n1b")


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE", "SFS2D_SLOTS_ONCE", "SFS2D_LEAN"):
        monkeypatch.delenv(k, raising=False)


def _engine():
    from sfs2d.engine import Engine
    return Engine.get(0)


def _setenv(monkeypatch, kind):
    for k, v in AU.KINDS[kind].get("env", {}).items():
        monkeypatch.setenv(k, v)


def _plan(kind, dev):
    """(base plan, the plan of the record calls) of a kind over ``dev``: the background supplied, the attached plan
    attached; not run."""
    pl = dev.eng.plan(dev, AU.scan_config(kind))
    try:
        if AU.KINDS[kind].get("supplied"):
            pl.set_background(*AU.supplied_background(kind))
        return pl, (pl.attach(AU.scan_config(kind, attached=True)) if "attach" in AU.KINDS[kind] else pl)
    except Exception:
        pl.close()
        raise


def _assert_kind(kind, pl):
    k = AU.KINDS[kind]
    assert pl.scan_kernel() == k["kernel"]
    v = pl.scan_variant()
    assert {f: v[f] for f in k["variant"]} == k["variant"], (kind, v)


def _selections(kind, nrec, nchrom):
    """(pooled groups of the spectra call, (rec, grp) of the chromosome-entry project call)."""
    return (np.arange(nrec) % 3).astype(np.int32), ([-(c + 1) for c in range(nchrom)], list(range(nchrom)))


def _calls(kind, pl, rpl, tasks=None):
    """The five calls and the two reads on a plan that has made its last run: {name: array}."""
    which = AU.which_of(kind)
    m = AU.sizes(kind)[1]
    tasks = AU.tasks(which, AU.KINDS[kind].get("supplied", False)) if tasks is None else tasks
    nchrom = AU.pair(which)[0].nchrom
    pooled, (crec, cgrp) = _selections(kind, rpl.nrec, nchrom)
    out = {}
    pl.null_run(tasks, AU.NULL_REPS, AU.NULL_SEED)
    out["null"] = pl.null_read()
    pl.null_run(tasks, AU.NULL_REPS, AU.NULL_SEED, block=AU.NULL_BLOCK)
    out["null_blocks"] = pl.null_read()
    out["diversity"] = rpl.diversity()
    out["spectra"] = rpl.spectra()
    out["spectra_pooled"] = rpl.spectra(None, pooled, 3)
    out["project"], out["project_used"], out["project_dropped"] = rpl.project(*m)
    out["project_e"] = np.array([rpl.project_e])
    out["project_chrom"], out["project_chrom_used"], out["project_chrom_dropped"] = rpl.project(*m, crec, cgrp, nchrom)
    out["project_chrom_e"] = np.array([rpl.project_e])
    out["read"], out["fst"] = rpl.read(), rpl.read_fst()
    if rpl is not pl:
        out["base_read"], out["base_fst"] = pl.read(), pl.read_fst()
    return out


def _same(got, want, what, failures=None):
    """Every array byte-equal to the control's; ``failures`` (a list): the mismatch is appended, not raised, so that a
    test of several rounds reports every round that differs."""
    assert list(got) == list(want)
    bad = [k for k in want if got[k].tobytes() != want[k].tobytes()]
    for i, k in enumerate(bad):
        if k.startswith("null"):      # (for the report: a few last bits, or another background altogether?)
            try:
                NU.check(got[k], want[k])
                bad[i] = k + " (within the twin's tolerance of the control)"
            except AssertionError:
                bad[i] = k + " (beyond the twin's tolerance of the control)"
    msg = f"{what}: differ from the control: {', '.join(bad)}"
    if bad and failures is not None:
        failures.append(msg)
    else:
        assert not bad, msg


def _check_control(kind, p, out, tasks, bg_of):
    """(b): the control's arrays against the twins."""
    m = AU.sizes(kind)[1]
    cfg, rcfg = AU.scan_config(kind), AU.record_config(kind)
    ocfg, rocfg = AU.oracle_cfg(cfg, p), AU.oracle_cfg(rcfg, p)
    what = f"control {kind}"
    want = NU.null_twin(p, tasks, AU.NULL_REPS, AU.NULL_SEED, ocfg, bg_of)[0]
    assert NU.check(out["null"], want) >= len(want)
    want = NU.oracle_records(*N.resample(p, tasks, AU.NULL_REPS, AU.NULL_SEED, block=AU.NULL_BLOCK), ocfg, bg_of)
    assert NU.check(out["null_blocks"], want) >= len(want)
    recs = out["read"]
    n = len(recs)
    slots, orec = AU.slot_records(kind, p)
    body = recs[(recs["flags"] & L.W_EXTRA) == 0]
    assert len(body) == len(slots)
    for r, s, o in zip(body, slots, orec):
        assert (o is None) == bool(r["flags"] & L.W_EMPTY), s
        if o is not None:
            want = (s[0], s[2], s[3], o["snp_count"], o["N2"], o["N2_all"], o["N1a"], o["N1b"])
            assert tuple(int(r[f]) for f in REC_INTS) == want, (s, r)
    DU.assert_records(out["diversity"], DU.expected_for_records(p, recs, rocfg), what)
    SU.assert_rows(out["spectra"][:n], SU.expected(p, recs, rocfg), what)
    pooled, (crec, cgrp) = _selections(kind, n, p.nchrom)
    SU.assert_rows(out["spectra_pooled"], SU.expected(p, recs, rocfg, None, pooled, 3), what + " pooled")
    e = int(out["project_e"][0])
    PU.assert_grids(out["project"][:n], out["project_used"][:n], out["project_dropped"][:n], PU.twin(p, recs, rcfg, *m), e, what)
    PU.assert_grids(out["project_chrom"], out["project_chrom_used"], out["project_chrom_dropped"],
                    PU.twin(p, recs, rcfg, *m, crec, cgrp, p.nchrom), int(out["project_chrom_e"][0]), what + " chromosomes")
    assert out["project_used"].sum() > 1000 and np.isfinite(out["fst"]).sum() >= 5


def _control(kind, p, rows=None):
    """The control's arrays for data set ``p`` (its environment is the caller's: call after _setenv); computed and
    checked against the twins once per (kind, data set), read-only.  ``rows`` (name, fn): a phase-split control --
    run(phase=1), its background rows through fn on the device, run(phase=2)."""
    key = (kind, id(p), rows[0] if rows else None)
    if key in _CONTROL:
        return _CONTROL[key]
    import torch
    eng = _engine()
    dev = eng.upload(p)
    try:
        pl, rpl = _plan(kind, dev)
        try:
            bg_of = AU.background_of(kind, p)
            if rows is None:
                pl.run()
            else:
                bg_of = _split_run(kind, pl, rows[1], None)
            pl.check()
            _assert_kind(kind, pl)
            tasks = AU.tasks(AU.which_of(kind), AU.KINDS[kind].get("supplied", False))
            out = _calls(kind, pl, rpl, tasks)
        finally:
            pl.close()
    finally:
        dev.close()
    torch.cuda.synchronize()
    if rows is None:
        _check_control(kind, p, out, tasks, bg_of)
    else:   # the null alone sees the exchanged background (the windows' T's are checked through read() by the caller)
        ocfg = AU.oracle_cfg(AU.scan_config(kind), p)
        want = NU.null_twin(p, tasks, AU.NULL_REPS, AU.NULL_SEED, ocfg, bg_of)[0]
        assert NU.check(out["null"], want) >= len(want)
        want = NU.oracle_records(*N.resample(p, tasks, AU.NULL_REPS, AU.NULL_SEED, block=AU.NULL_BLOCK), ocfg, bg_of)
        assert NU.check(out["null_blocks"], want) >= len(want)
    for a in out.values():
        a.setflags(write=False)
    _CONTROL[key] = out
    return out


def _split_run(kind, pl, fn, out_ptr):
    """run(phase=1); the plan's background rows to a device buffer, through ``fn`` (None: no exchange at all) and
    back; run(out_ptr, phase=2).  Returns bg_of(chrom) of the rows written back (None without an exchange)."""
    import ctypes as C
    import torch
    eng = pl.eng
    cfg = AU.scan_config(kind)
    nchrom = AU.pair(AU.which_of(kind))[0].nchrom
    W = L.bg_row_words(cfg.n1p, cfg.n2p)
    pl.run(phase=1)
    bg_of = None
    if fn is not None:
        buf = torch.zeros((nchrom, W), dtype=torch.int64, device=f"cuda:{eng.device}")
        torch.cuda.synchronize()
        eng.check(eng.lib.sfs2d_plan_bg_rows_dev(pl.h, C.c_void_p(buf.data_ptr()), W))
        pl.check()                                   # (synchronises the engine's stream: torch reads the rows next)
        new = fn(buf).contiguous()
        torch.cuda.synchronize()
        eng.check(eng.lib.sfs2d_plan_bg_rows_set_dev(pl.h, C.c_void_p(new.data_ptr()), W))
        bg_of = SPL.backgrounds_of_rows(cfg, new.cpu().numpy())
        pl.run(out_ptr, phase=2)
        pl.check()                                   # (the rows are read before ``new`` goes)
    else:
        pl.run(out_ptr, phase=2)
    return bg_of


def _rows_of(kind, p):
    """The background rows [nchrom, SFS2D_BG_ROW_WORDS] of a kind's plan over an upload of ``p``, on the device."""
    if (kind, id(p)) not in _ROWS:
        eng = _engine()
        dev = eng.upload(p)
        try:
            pl, _ = _plan(kind, dev)
            try:
                keep = []
                _split_run(kind, pl, lambda t: keep.append(t.clone()) or t, None)
            finally:
                pl.close()
        finally:
            dev.close()
        _ROWS[(kind, id(p))] = keep[0]
    return _ROWS[(kind, id(p))]


class Subject:
    """``nplans`` plans of a kind over ONE wrapped data set holding A, each run once and checked."""

    def __init__(self, kind, nplans=1, run=True):
        self.kind = kind
        self.a, self.b = AU.pair(AU.which_of(kind))
        self.w = AU.Wrapped(_engine(), self.a, ann=AU.KINDS[kind].get("ann", False))
        self.plans = []
        try:
            for _ in range(nplans):
                self.plans.append(_plan(kind, self.w.dev))
            for pl, _ in self.plans if run else []:
                pl.run()
                pl.check()
                _assert_kind(kind, pl)
        except Exception:
            self.close()
            raise

    def buffer(self, k=0):
        import torch
        t = torch.zeros((max(1, self.plans[k][0].nrec), 64), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        return t

    def check(self, what, want=None, failures=None):
        """Synchronise everything, then every plan's calls against the control of the data the arrays hold now."""
        import torch
        torch.cuda.synchronize()
        want = _control(self.kind, self.w.now) if want is None else want
        for k, (pl, rpl) in enumerate(self.plans):
            pl.check()
            _same(_calls(self.kind, pl, rpl), want, f"{self.kind}: {what}, plan {k}", failures)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def close(self):
        import torch
        torch.cuda.synchronize()
        for pl, _ in self.plans:
            pl.close()
        self.plans = []
        self.w.close()


def _records(buf, pl):
    return np.frombuffer(buf.cpu().numpy().tobytes(), dtype=L.WINDOW_DTYPE)[: pl.nrec]


# ------------------------------------------------------------------------------------------------- the routes

@pytest.mark.parametrize("kind", list(AU.KINDS))
def test_after_run_into_a_caller_buffer(monkeypatch, kind):
    """1: the caller's buffer holds B's records, the plan's own A's: the calls and read() follow the buffer."""
    _setenv(monkeypatch, kind)
    with Subject(kind) as s:
        pl = s.plans[0][0]
        own = pl.read()
        s.w.rewrite(s.b)
        buf = s.buffer()
        pl.run(buf.data_ptr())
        s.check("run(out_dev_ptr)")
        got = _records(buf, pl)
        assert got.tobytes() == pl.read().tobytes() and got.tobytes() != own.tobytes()
        pl.run()                                     # and back into the plan's own buffer, on A
        s.w.rewrite(s.a)
        pl.run()
        s.check("run() after run(out_dev_ptr)")
        assert _records(buf, pl).tobytes() == got.tobytes()


@pytest.mark.parametrize("kind", AU.EVERY_ROUTE)
def test_after_run_many(monkeypatch, kind):
    """2: 1 + 2 runs (the last of parity 0) into a caller's buffer, then 3 more (parity 1) into the plan's own."""
    _setenv(monkeypatch, kind)
    with Subject(kind) as s:
        pl = s.plans[0][0]
        s.w.rewrite(s.b)
        buf = s.buffer()
        pl.run_many(2, buf.data_ptr())
        s.check("run_many(2, buf)")
        s.w.rewrite(s.a)
        pl.run_many(3)
        s.check("run_many(3)")


@pytest.mark.parametrize("streams", ["engine", "torch"])
@pytest.mark.parametrize("kind", AU.EVERY_ROUTE)
def test_after_run_streams(monkeypatch, kind, streams):
    """3: two plans; 3 runs (the staggered start: plan 0 runs twice, plan 1 once) and then 4."""
    import torch
    from sfs2d.engine import Plan
    _setenv(monkeypatch, kind)
    with Subject(kind, nplans=2) as s:
        base = [pl for pl, _ in s.plans]
        st = [None, None] if streams == "engine" else [torch.cuda.Stream(device=0).cuda_stream for _ in range(2)]
        s.w.rewrite(s.b)
        Plan.run_streams(base, st, 3)
        s.check("run_streams(3)")
        s.w.rewrite(s.a)
        buf = s.buffer(1)
        Plan.run_streams(base, st, 4, [None, buf.data_ptr()])
        s.check("run_streams(4)")
        assert _records(buf, base[1]).tobytes() == base[1].read().tobytes()


@pytest.mark.parametrize("kind", list(AU.KINDS))
def test_after_graph_replay(monkeypatch, kind):
    """4: a replay is the plan's last run, a capture is not.  Two plans captured on two streams, plan 1 into a caller's
    buffer.  Before any launch the calls still see the runs before the capture (and complete the null's tables for
    them); then the graph is replayed on B, twice on A, and once more on A without a rewrite (a sliced plan's tables
    then lack their tail unless the null completes them again after every replay); then plan 1 runs twice on its own
    (into its own buffer) and a replay on B follows: the calls go back to the captured buffer.  Every round that
    differs from the control is reported."""
    import torch
    from sfs2d.engine import Plan
    _setenv(monkeypatch, kind)
    with Subject(kind, nplans=2) as s:
        base = [pl for pl, _ in s.plans]
        streams = [torch.cuda.Stream(device=0) for _ in range(2)]
        buf = s.buffer(1)
        g = Plan.graph(base, [x.cuda_stream for x in streams], 4, [None, buf.data_ptr()])
        bad = []
        try:
            s.check("captured, not launched: the runs before the capture", failures=bad)    # (A's, in the plans' own buffers)
            for p, n, what in ((s.b, 1, "launch(1) on B"), (s.a, 2, "launch(2) on A"), (None, 1, "launch(1) again")):
                if p is not None:
                    s.w.rewrite(p)
                g.launch(n)
                s.check(what, failures=bad)
                assert _records(buf, base[1]).tobytes() == _control(kind, s.w.now)["base_read" if "attach" in AU.KINDS[kind]
                                                                                    else "read"].tobytes(), what
            base[1].run()
            base[1].run()
            s.w.rewrite(s.b)
            g.launch(1)
            s.check("launch(1) on B after two runs into the plan's own buffer", failures=bad)
            assert not bad, "\n".join(bad)
        finally:
            torch.cuda.synchronize()
            g.close()


@pytest.mark.parametrize("rows", ["none", "doubled", "other"])
@pytest.mark.parametrize("kind", AU.EVERY_ROUTE)
def test_after_phase_split_run(monkeypatch, kind, rows):
    """5: run(phase=1), run(buf, phase=2).  Without an exchange it is a run.  With the plan's rows doubled the windows'
    T's are the plain control's (T does not see a scale) and the null equals a control whose background is the
    doubled rows.  With the rows of the OTHER data set written back (what an all-reduce does: the background is not
    the part's own) windows and null are evaluated against A's backgrounds on B's SNPs: the null after a split run
    uses the exchanged rows."""
    import torch
    _setenv(monkeypatch, kind)
    a, b = AU.pair(AU.which_of(kind))
    fn, want = None, None
    if rows == "doubled":
        fn = lambda t: t * 2
    elif rows == "other":
        other = _rows_of(kind, a)
        fn = lambda t: other.clone()
    if fn is not None:
        want = _control(kind, b, (rows, fn))
    with Subject(kind) as s:
        pl = s.plans[0][0]
        s.w.rewrite(s.b)
        buf = s.buffer()
        _split_run(kind, pl, fn, buf.data_ptr())
        s.check(f"phase split, rows {rows}", want)
        assert _records(buf, pl).tobytes() == pl.read().tobytes()
    plain = _control(kind, b)
    if rows == "doubled":      # T does not see a scale of the background: the plain control's records, Fst byte-equal
        for f in NU.INTS:
            assert np.array_equal(want["read"][f], plain["read"][f]), f
        for f in ("t2d", "t1d_p1", "t1d_p2"):
            assert all(gu.close(float(x), float(y), scale=NU.T_FLOOR) for x, y in zip(want["read"][f], plain["read"][f])), f
        assert want["fst"].tobytes() == plain["fst"].tobytes()
    if rows == "other":
        live = (plain["read"]["flags"] & L.W_EMPTY) == 0
        assert np.array_equal(want["read"]["n2"], plain["read"]["n2"])
        assert 2 * (want["read"]["t2d"][live] != plain["read"]["t2d"][live]).sum() > live.sum()
        assert 2 * (want["null"]["t2d"] != plain["null"]["t2d"]).sum() > len(plain["null"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", AU.EVERY_ROUTE)
def test_after_plan_time(monkeypatch, kind):
    """6: sfs2d_plan_time writes the plan's own buffer, whatever the run before it wrote."""
    _setenv(monkeypatch, kind)
    with Subject(kind) as s:
        pl = s.plans[0][0]
        buf = s.buffer()
        pl.run(buf.data_ptr())
        pl.check()
        s.w.rewrite(s.b)
        pl.time(2)
        s.check("time(2)")


@pytest.mark.parametrize("kind", AU.EVERY_ROUTE)
def test_captured_and_never_executed(monkeypatch, kind):
    """A capture enqueues nothing: the plan has no last run until the graph is launched."""
    import torch
    from sfs2d.engine import Plan
    _setenv(monkeypatch, kind)
    m = AU.sizes(kind)[1]
    with Subject(kind, run=False) as s:
        pl = s.plans[0][0]
        stream = torch.cuda.Stream(device=0)
        g = Plan.graph([pl], [stream.cuda_stream], 2)
        try:
            calls = {"null_run": lambda: pl.null_run([(0, 5)], 3, 1), "null_run_blocks": lambda: pl.null_run([(0, 5)], 3, 1, block=4),
                     "diversity": pl.diversity, "spectra": pl.spectra, "project": lambda: pl.project(*m), "read": pl.read,
                     "read_fst": pl.read_fst}
            for name, call in calls.items():
                with pytest.raises(L.Sfs2dError) as ei:
                    call()
                assert ei.value.code == L.E_ARG and "run" in str(ei.value), (name, str(ei.value))
            g.launch(1)
            s.check("launch(1) of a plan that never ran")
            _assert_kind(kind, pl)
        finally:
            torch.cuda.synchronize()
            g.close()
