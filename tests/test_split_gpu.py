"""The phase-split background exchange (sfs2d_plan_run_phase 1 / 2 around sfs2d_plan_bg_rows_dev / _set_dev, or
sfs2d_plan_bg_exchange on the host) pinned to the oracle in one process: K plans on one engine stand in for K
ranks (tests/split_util.py), ~9,200 SNPs.

  a  the exchanged rows word for word against the oracle's, at n1p != n2p, with filters, with a padded stride
  b  records and Fst of the merged table against the oracle with the WHOLE data set's backgrounds, on every
     scan path; byte-equal to one whole plan's table
  c  a split on a plan that has run (odd buffer parity), an ordinary run after a split, a split after that
  d  a plan attached to a split base
  e  parts whose own inner sums are 0 while the total's are not, and the reverse
  f  overflowing sums: SFS2D_E_ARG from check(), and the plan recovers
  g  the host form of the exchange
  h  sfs2d_bg_hist_dev per chromosome

Rows and every integer field exact, T2D / T1D by golden_util.close, Fst within 1e-12 + 1e-10 |x| (wide_util)."""
import ctypes as C

import numpy as np
import pytest

import dist_worker as DW
import golden_util as gu
import split_util as SU
import wide_util as U
from oracle import sfs_oracle as O

pytestmark = pytest.mark.gpu

CASES = SU.all_cases()
FLAVOURS = {"fused": ({"SFS2D_FUSED": "1"}, 25, 25), "sliced": ({"SFS2D_FUSED": "0"}, 25, 25),
            "g": ({"SFS2D_GW": "0"}, 60, 35), "gw": ({"SFS2D_GW": "1"}, 60, 35)}
REPL = 4   # sfs2d_kernels.hpp


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE", "SFS2D_WGS", "SFS2D_LNL"):
        monkeypatch.delenv(k, raising=False)


def _eng():
    from sfs2d.engine import Engine
    return Engine.get(0)


def _setenv(monkeypatch, flavour):
    for k, v in FLAVOURS[flavour][0].items():
        monkeypatch.setenv(k, v)


def _ref(name):
    """The oracle's (windows, records, Fst) of the whole data set against its own per-chromosome backgrounds."""
    p, cfg = CASES[name]
    ocfg = SU.ocfg_of(p, cfg)
    if ("split", name) not in U._REF:
        bgs = O.chrom_backgrounds(p, ocfg)
        U.oracle_ref(p, SU.windows(p, cfg), ocfg, lambda c: bgs[c], key=("split", name))
    return U._REF[("split", name)]


def _fake(name, cname="four"):
    p, cfg = CASES[name]
    return SU.fake_split((name, cname), p, cfg, SU.cut_lists(p, cfg)[cname])


def _whole(p, cfg, wrap=False):
    """One plan over the whole data set: its records."""
    job = SU.GpuSplitJob(_eng(), p, cfg, wrap=wrap)
    try:
        return job.whole()[0]
    finally:
        job.close()


def _body(t):
    from sfs2d import _lib as L
    return t[(t["flags"] & L.W_EXTRA) == 0]


def _check_rows(res, fake):
    """Every part's rows are the oracle's, word for word (the inner-sum word is the last)."""
    assert len(res.rows) == len(fake.rows)
    for r, (got, want) in enumerate(zip(res.rows, fake.rows)):
        assert (got is None) == (want is None), r
        if got is not None:
            W = want.shape[1]
            bad = np.argwhere(got[:, :W] != want)
            assert bad.size == 0, (r, bad[:5], [int(got[i, k]) for i, k in bad[:5]], [int(want[i, k]) for i, k in bad[:5]])
    assert np.array_equal(res.total[:, : fake.total.shape[1]], fake.total)


def _check_table(name, res, whole=None):
    """The merged table: every window against the oracle (whole-data backgrounds), every integer field and flag
    of every window equal to the oracle's table (fake_records), the Q9 helper's 1D fields too; with ``whole``
    byte-equal to one plan's table."""
    from sfs2d import _lib as L
    p, cfg = CASES[name]
    U.check_records(res.table, res.merged_fst(), _ref(name))
    got, want = SU.strip(res.table), SU.strip(_fake(name).table)
    U.same_ints(_body(got), _body(want))
    g, w = got[(got["flags"] & L.W_EXTRA) != 0], want[(want["flags"] & L.W_EXTRA) != 0]
    assert len(g) == len(w) == int(bool(cfg.prev_extra))
    for a, b in zip(g, w):
        for k in ("chrom", "begin", "end", "n1a", "n1b", "flags"):
            assert int(a[k]) == int(b[k]), (k, int(a[k]), int(b[k]))
        for k, z in (("t1d_p1", L.W_BG1A_ZERO), ("t1d_p2", L.W_BG1B_ZERO)):
            v = float(a[k])
            if int(b["flags"]) & z:   # no background: the oracle's None (0 or NaN in the record)
                assert v == 0.0 or np.isnan(v), (k, v)
            else:
                assert gu.close(v, float(b[k])), (k, v, float(b[k]))
    if whole is not None:
        assert got.tobytes() == SU.strip(whole).tobytes()


def _split(name, cname="four", wrap=False, attach=None, **kw):
    p, cfg = CASES[name]
    return SU.split_in_process(p, cfg, SU.cut_lists(p, cfg)[cname], SU.GpuJobs(_eng(), wrap=wrap, attach=attach), **kw)


# ------------------------------------------------------------------------------------------------------ a. rows

@pytest.mark.parametrize("variant", ["fold", "nofold", "ann", "pos"])
@pytest.mark.parametrize("n1p,n2p", SU.GRIDS_ROWS)
def test_rows_equal_the_oracle(n1p, n2p, variant):
    """After phase 1 every part's sfs2d_plan_bg_rows_dev rows are FakeSplitJob.partial() of that part; the merged
    table is the oracle's."""
    name = f"rows-{n1p}x{n2p}-{variant}"
    res = _split(name)
    try:
        _check_rows(res, _fake(name))
        _check_table(name, res)
    finally:
        res.close()


@pytest.mark.parametrize("n1p,n2p", SU.GRIDS_ROWS)
def test_rows_padded_stride(n1p, n2p):
    """stride = W + 5, padding -1: k_bg_rows_get leaves the five padding words of every row alone, and
    k_bg_rows_set ignores them (they sum to -4: read as data they would be an overflow)."""
    name = f"rows-{n1p}x{n2p}-nofold"
    p, cfg = CASES[name]
    from sfs2d import dist as D
    W = D.hist_width(cfg)
    res = _split(name, stride=W + 5)
    try:
        assert res.buffer.shape == (4, 3, W + 5)
        assert np.all(res.buffer[:, :, W:] == -1) and np.all(res.total[:, W:] == -4)
        _check_rows(res, _fake(name))
        _check_table(name, res)
    finally:
        res.close()


# ----------------------------------------------------------------------------------- b. records after the exchange

@pytest.mark.parametrize("cname", ["four", "empty"])
@pytest.mark.parametrize("fst", [False, True])
@pytest.mark.parametrize("win", ["bp20k", "snp500"])
@pytest.mark.parametrize("flavour", ["fused", "sliced"])
def test_scan_w_after_the_exchange(monkeypatch, flavour, win, fst, cname):
    _setenv(monkeypatch, flavour)
    name = f"w-{win}-fst{int(fst)}"
    p, cfg = CASES[name]
    res = _split(name, cname)
    try:
        for j in res.jobs:
            if j is not None:
                assert j.pl.scan_kernel() == "k_scan_w"
                assert j.pl.scan_variant()["fused"] == (1 if flavour == "fused" else 0)
        _check_rows(res, _fake(name, cname))
        _check_table(name, res, _whole(p, cfg))
    finally:
        res.close()


@pytest.mark.parametrize("cname", ["four", "empty"])
@pytest.mark.parametrize("n1p,n2p", SU.GRIDS_LARGE)
@pytest.mark.parametrize("gw", [0, 1])
def test_large_grid_after_the_exchange(monkeypatch, gw, n1p, n2p, cname):
    """k_scan_g / k_scan_gw: launch_bg_slices builds the tables from the exchanged replica 0 in phase 2."""
    monkeypatch.setenv("SFS2D_GW", str(gw))
    name = f"large-{n1p}x{n2p}"
    p, cfg = CASES[name]
    res = _split(name, cname)
    try:
        for j in res.jobs:
            if j is not None:
                assert j.pl.scan_kernel() == ("k_scan_gw" if gw else "k_scan_g")
        _check_rows(res, _fake(name, cname))
        _check_table(name, res, _whole(p, cfg))
    finally:
        res.close()


@pytest.mark.parametrize("cname", ["four", "empty"])
def test_wide_bins_after_the_exchange(cname):
    """Device arrays without host positions and 70 kb windows: 32-bit 2D bins (P16 = false) in phase 2."""
    name = "wide-70k"
    p, cfg = CASES[name]
    res = _split(name, cname, wrap=True)
    try:
        for j in res.jobs:
            if j is not None:
                assert j.pl.scan_variant()["p16"] == 0
        _check_rows(res, _fake(name, cname))
        _check_table(name, res, _whole(p, cfg, wrap=True))
    finally:
        res.close()


# --------------------------------------------------------------------------------------------- c. reuse and parity

@pytest.mark.parametrize("flavour", ["fused", "sliced", "gw"])
def test_reuse_and_parity(monkeypatch, flavour):
    """A split on plans that have run once (odd parity) is the split on fresh plans, byte for byte; after a split
    an ordinary run of each part's plan gives the oracle's records of that part alone against its own backgrounds;
    a split after that, and one more straight after it (odd parity, after a split), give the first split's bytes."""
    _setenv(monkeypatch, flavour)
    _, n1p, n2p = FLAVOURS[flavour]
    name = "w-bp20k-fst1" if (n1p, n2p) == (25, 25) else f"large-{n1p}x{n2p}"
    p, cfg = CASES[name]
    cuts = SU.four_cuts(p, cfg)
    res0 = _split(name)
    try:
        _check_table(name, res0)
        res1 = _split(name, prior_runs=1)
        try:
            assert res1.table.tobytes() == res0.table.tobytes()
            assert [f.tobytes() for f in res1.fst] == [f.tobytes() for f in res0.fst]
        finally:
            res1.close()
        for r, job in enumerate(res0.jobs):
            sub = res0.subs[r]
            with SU.on_stream(job.eng):
                recs, fst = job.whole()
            ocfg = SU.ocfg_of(sub, job.cfg)
            bgs = O.chrom_backgrounds(sub, ocfg)
            U.check_against_oracle(recs, fst, sub, SU.windows(sub, job.cfg), ocfg, lambda c: bgs[c],
                                   key=("split-part", name, r))
        for again in (1, 2):
            res2 = SU.split_in_process(p, cfg, cuts, SU.Reuse(res0))
            assert res2.table.tobytes() == res0.table.tobytes(), again
            assert [f.tobytes() for f in res2.fst] == [f.tobytes() for f in res0.fst], again
            assert np.array_equal(res2.buffer, res0.buffer), again
    finally:
        res0.close()


# ------------------------------------------------------------------------------------------------- d. attached

@pytest.mark.parametrize("flavour", ["fused", "sliced"])
def test_attached_plan_on_a_split_base(monkeypatch, flavour):
    """Base 20 kb with Fst, a 100 kb plan with Fst attached, cuts at 100 kb window starts: launch_attached scans
    from the base's exchanged tables; the parts' attached tables merge to the oracle's 100 kb table."""
    from sfs2d import _lib as L
    from sfs2d import dist as D
    _setenv(monkeypatch, flavour)
    p, acfg = CASES["attach-100k"]
    cfg = CASES["w-bp20k-fst1"][1]
    cuts = SU.four_cuts(p, acfg)
    res = SU.split_in_process(p, cfg, cuts, SU.GpuJobs(_eng(), attach=acfg))
    try:
        U.check_records(res.table, res.merged_fst(), _ref("w-bp20k-fst1"))
        tabs, fsts = [], []
        for j in res.jobs:
            t, f = j.attached()
            tabs.append(t)
            fsts.append(f[(t["flags"][: len(f)] & L.W_EMPTY) == 0])
        merged = D._merge_split(tabs, cuts, res.c0s, False, 0, p.chrom_off)
        U.check_records(merged, np.concatenate(fsts), _ref("attach-100k"))
        U.same_ints(SU.strip(merged), SU.strip(_fake("attach-100k").table))
    finally:
        res.close()


# ----------------------------------------------------------------------------------------- e. background-zero cases

@pytest.mark.parametrize("flavour", ["fused", "sliced"])
@pytest.mark.parametrize("name", ["corner_part", "zero_chrom", "end_filter"])
def test_background_zero_flags_come_from_the_total(monkeypatch, name, flavour):
    """corner_part: part 2's own inner sums are 0 (asserted on its rows), its windows carry no BG*_ZERO flag;
    zero_chrom: chromosome 1's total inner 2D sum is 0 over two parts, every window of it carries BG2_ZERO in both;
    end_filter: part 2's rows are all 0 and its windows are evaluated against the total.  Flags and integers are
    the oracle's table's (fake_records), T the oracle's against the whole chromosome."""
    from sfs2d import _lib as L
    _setenv(monkeypatch, flavour)
    p, cfg = CASES[name]
    res = _split(name)
    try:
        _check_rows(res, _fake(name))
        if name == "corner_part":
            assert res.rows[2][0, -1] == 0 and res.rows[2][0].sum() > 0 and res.total[1, -1] > 0
        elif name == "zero_chrom":
            assert res.total[1, -1] == 0 and res.rows[1][0, -1] > 0
        else:
            assert not res.rows[2].any() and res.total[1, -1] > 0
        _check_table(name, res, _whole(p, cfg))
        t = _body(res.table)
        on1 = t["chrom"] == 1
        want = (L.W_BG2_ZERO | L.W_BG1A_ZERO | L.W_BG1B_ZERO) if name == "zero_chrom" else 0
        assert on1.sum() >= 4 and np.all(t["flags"][on1] & 7 == want) and np.all(t["flags"][~on1] & 7 == 0)
    finally:
        res.close()


# ------------------------------------------------------------------------------------------------- f. overflow

def _part1(name):
    """Part 1 of the four-part cuts (the end of chromosome 0 and the start of chromosome 1), its oracle rows and
    the totals of its two chromosomes."""
    p, cfg = CASES[name]
    fake = _fake(name)
    assert fake.c0s[1] == 0 and fake.subs[1].nchrom == 2
    return fake.subs[1], fake.jobs[1].cfg, fake.rows[1], fake.total[0:2]


def _check_part(recs, fst, sub, cfg, total):
    """A part's records against the oracle's with the backgrounds of the summed rows."""
    U.check_against_oracle(recs, fst, sub, SU.windows(sub, cfg), SU.ocfg_of(sub, cfg), SU.backgrounds_of_rows(cfg, total))


def test_overflow_is_reported_and_cleared():
    """A summed word of 2^32, or of -1: check() raises SFS2D_E_ARG with the overflow message (phase 2 not run);
    0xffffffff in 2D bin 0 passes; then the true sums, phase 2, and the oracle's records: the error word was
    cleared and the plan recovered."""
    import torch
    from sfs2d import _lib as L
    sub, cfg, rows, total = _part1("w-bp20k-fst1")
    W = rows.shape[1]
    eng = _eng()
    with SU.on_stream(eng):
        job = SU.GpuSplitJob(eng, sub, cfg)
        try:
            mine = torch.zeros((2, W), dtype=torch.int64, device="cuda:0")
            job.partial_dev(mine.data_ptr(), W)
            assert np.array_equal(mine.cpu().numpy(), rows)
            tot = torch.from_numpy(np.ascontiguousarray(total)).to("cuda:0")
            k2 = int(np.argmax(total[1, 1:51 * 51 - 1])) + 1   # an inner 2D bin of chromosome 1
            for (c, k), v in (((1, k2), 1 << 32), ((0, 51 * 51 + 3), -1), ((1, W - 1), 1 << 32)):
                bad = tot.clone()
                bad[c, k] = v
                job.rows_set(bad.data_ptr(), W)
                with pytest.raises(L.Sfs2dError) as ei:
                    job.pl.check()
                assert ei.value.code == L.E_ARG and "overflow" in str(ei.value), (c, k, v)
                job.pl.check()   # (reported once)
            edge = tot.clone()
            edge[0, 0] = 0xFFFFFFFF
            job.rows_set(edge.data_ptr(), W)
            job.pl.check()
            job.rows_set(tot.data_ptr(), W)
            recs = job.phase2()
            _check_part(recs, job.fst(), sub, cfg, total)
        finally:
            job.close()


# ------------------------------------------------------------------------------------------- g. host exchange

def _words(job):
    v = [C.c_int64() for _ in range(3)]
    job.eng.check(job.eng.lib.sfs2d_plan_bg_words(job.pl.h, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _exchange(job, repl, sums, to_device):
    from sfs2d import _lib as L
    job.eng.check(job.eng.lib.sfs2d_plan_bg_exchange(job.pl.h, L.ptr(repl), L.ptr(sums), int(to_device)))


@pytest.mark.parametrize("prior", [0, 1])
@pytest.mark.parametrize("flavour", ["fused", "sliced", "gw"])
def test_host_exchange(monkeypatch, flavour, prior):
    """sfs2d_plan_bg_words / _bg_buffer / _bg_exchange on part 1: the replicas read after phase 1 sum to the
    bg_rows_dev rows; totals written back with to_device = 1 give, after phase 2, the records of the
    bg_rows_set_dev route byte for byte; after bg_rows_set_dev replica 0 holds the totals and the others 0."""
    import torch
    _setenv(monkeypatch, flavour)
    _, n1p, n2p = FLAVOURS[flavour]
    sub, cfg, rows, total = _part1("w-bp20k-fst1" if (n1p, n2p) == (25, 25) else f"large-{n1p}x{n2p}")
    W = rows.shape[1]
    eng = _eng()
    with SU.on_stream(eng):
        a, b = SU.GpuSplitJob(eng, sub, cfg), SU.GpuSplitJob(eng, sub, cfg)
        try:
            R, nc, nh = _words(a)
            assert (R, nc, nh) == (REPL, 2, (W - 1 + 3) & ~3)
            for job in (a, b):
                for _ in range(prior):
                    job.whole()
            assert a.pl.bg_buffer()[1] == R * nc * nh * 4
            # a: the host route
            a.pl.run(phase=1)
            got = torch.full((2, W), -1, dtype=torch.int64, device="cuda:0")
            a.rows_get(got.data_ptr(), W)
            got = got.cpu().numpy()
            assert np.array_equal(got, rows)
            repl, sums = np.full((R, nc, nh), 7, np.uint32), np.full(nc, 7, np.uint32)
            _exchange(a, repl, sums, 0)
            assert np.array_equal(repl.astype(np.int64).sum(0)[:, : W - 1], rows[:, : W - 1])
            assert np.array_equal(sums.astype(np.int64), rows[:, -1])
            back = np.zeros((R, nc, nh), np.uint32)
            back[0, :, : W - 1] = total[:, : W - 1]
            _exchange(a, back, np.ascontiguousarray(total[:, -1].astype(np.uint32)), 1)
            seen = torch.full((2, W), -1, dtype=torch.int64, device="cuda:0")
            a.rows_get(seen.data_ptr(), W)
            assert np.array_equal(seen.cpu().numpy(), total)
            ra, fa = a.phase2(), a.fst()
            # b: the device route, and what k_bg_rows_set left in the replicas
            mine = torch.zeros((2, W), dtype=torch.int64, device="cuda:0")
            b.partial_dev(mine.data_ptr(), W)
            tot = torch.from_numpy(np.ascontiguousarray(total)).to("cuda:0")
            b.rows_set(tot.data_ptr(), W)
            repl, sums = np.full((R, nc, nh), 7, np.uint32), np.full(nc, 7, np.uint32)
            _exchange(b, repl, sums, 0)
            assert np.array_equal(repl[0, :, : W - 1].astype(np.int64), total[:, : W - 1]) and not repl[0, :, W - 1:].any()
            assert not repl[1:].any() and np.array_equal(sums.astype(np.int64), total[:, -1])
            rb, fb = b.phase2(), b.fst()
            assert ra.tobytes() == rb.tobytes() and fa.tobytes() == fb.tobytes()
            _check_part(ra, fa, sub, cfg, total)
        finally:
            a.close()
            b.close()


def test_exchange_refusals():
    """SFS2D_E_ARG: an attached plan (exchange the base's), a supplied-background plan (nothing to exchange; its
    bg_words are zeros), a stride below the row width."""
    import torch
    from sfs2d import _lib as L
    from sfs2d.engine import ScanConfig
    sub, cfg, rows, total = _part1("w-bp20k-fst1")
    W = rows.shape[1]
    eng = _eng()
    lib = eng.lib
    bg = (np.arange(51 * 51, dtype=np.float64).reshape(51, 51) % 7 + 1, np.arange(26.0) + 1, np.arange(26.0) % 5 + 1)
    with SU.on_stream(eng):
        base = SU.GpuSplitJob(eng, sub, cfg, attach=CASES["attach-100k"][1])
        sup = SU.GpuSplitJob(eng, sub, ScanConfig(n1p=25, n2p=25, bg_mode=L.BG_SUPPLIED), bg=bg)
        try:
            buf = torch.zeros((2, W), dtype=torch.int64, device="cuda:0")
            repl, sums = np.zeros((REPL, 2, W + 1), np.uint32), np.zeros(2, np.uint32)
            assert _words(sup) == (0, 0, 0) and sup.pl.bg_buffer()[1] == 0
            base.pl.run(phase=1)

            def refused(rc):
                with pytest.raises(L.Sfs2dError) as ei:
                    eng.check(rc)
                assert ei.value.code == L.E_ARG

            for h in (base.att.h, sup.pl.h):
                refused(lib.sfs2d_plan_bg_rows_dev(h, C.c_void_p(buf.data_ptr()), W))
                refused(lib.sfs2d_plan_bg_rows_set_dev(h, C.c_void_p(buf.data_ptr()), W))
                refused(lib.sfs2d_plan_bg_exchange(h, L.ptr(repl), L.ptr(sums), 0))
                refused(lib.sfs2d_plan_bg_exchange(h, L.ptr(repl), L.ptr(sums), 1))
            refused(lib.sfs2d_plan_bg_rows_dev(base.pl.h, C.c_void_p(buf.data_ptr()), W - 1))
            refused(lib.sfs2d_plan_bg_rows_set_dev(base.pl.h, C.c_void_p(buf.data_ptr()), W - 1))
            refused(lib.sfs2d_plan_bg_rows_dev(base.pl.h, None, W))
            assert not buf.cpu().numpy().any()
            # the run in progress is still good: rows, totals, phase 2
            base.rows_get(buf.data_ptr(), W)
            assert np.array_equal(buf.cpu().numpy(), rows)
            tot = torch.from_numpy(np.ascontiguousarray(total)).to("cuda:0")
            base.rows_set(tot.data_ptr(), W)
            _check_part(base.phase2(), base.fst(), sub, cfg, total)
        finally:
            base.close()
            sup.close()


# ------------------------------------------------------------------------------------------- h. sfs2d_bg_hist_dev

@pytest.mark.parametrize("variant", ["plain", "filtered"])
@pytest.mark.parametrize("n1p,n2p", SU.GRIDS_ROWS[1:])
def test_bg_hist_dev_rows(n1p, n2p, variant):
    """chrom = 0, 1, 2 and -1: the row is the oracle's (for -1 the sum over the chromosomes); for chrom = c also
    the sum of the split parts' rows of chromosome c."""
    import torch
    name = f"rows-{n1p}x{n2p}-fold" if variant == "plain" else f"hist-{n1p}x{n2p}"
    p, cfg = CASES[name]
    want = DW.FakeSplitJob(p, cfg, None).partial()
    if variant == "filtered":
        plain = DW.FakeSplitJob(p, CASES[f"rows-{n1p}x{n2p}-fold"][1], None).partial()
        assert 0 < want[0, -1] < plain[0, -1] and 0 < want[1, -1] < plain[1, -1]
    W = want.shape[1]
    res = _split(name)
    res.close()
    assert np.array_equal(res.total, want)
    eng = _eng()
    with SU.on_stream(eng):
        d = eng.upload(p)
        try:
            for c in (0, 1, 2, -1):
                row = torch.full((W + 3,), -7, dtype=torch.int64, device="cuda:0")
                eng.bg_hist_dev(d, cfg, c, row.data_ptr())
                got = row.cpu().numpy()
                assert np.all(got[W:] == -7)
                assert np.array_equal(got[:W], want.sum(0) if c < 0 else want[c]), c
                if c >= 0:
                    assert np.array_equal(got[:W], res.total[c]), c
        finally:
            d.close()
