"""The null of the projected scan on the device (k_pnull_keys, k_pnull_heads, k_proj_null; sfs2d_plan_project_null;
DESIGN.md section 20), checked per replicate record against the host twin of the DRAWS (sfs2d.projnull) and the
device's own projection of the drawn SNPs:

* the integer link, exact: a 1-SNP SNP-count-window plan on the same data gives one record per SNP, so
  ``Plan.project(m1, m2, rec=<the twin's drawn SNPs>, grp=<replicate ids>)`` yields each replicate's grid as integer sums
  at 2^-e rounded by the same device code; n2_fx, n1a_fx, n1b_fx must equal projscan_util.fixed_sums of those grids,
  n_used, n_dropped and e the observed record's, and the two calls report the same e;
* the arithmetic: t2d, t1d_p1, t1d_p2 against projscan_util.closed_form of those grids and the chromosome-entry grid
  within 1e-10 A (section 19's tolerance), NaN and +inf at the same records;
* n_thin against the twin.

The genome is projscan_util's (chromosomes of 1 .. 9,000 SNPs, 18 / 14, 2 % missing, an all-dropped 3-SNP window)."""
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
from sfs2d import projnull as PN
from sfs2d import spectra as SP

pytestmark = pytest.mark.gpu

N1P, N2P = 18, 14
M = (24, 20)
FILT = {"start_position": 3000, "end_position": 400000, "ann_want": 1}
FIELDS = ("t2d", "t1d_p1", "t1d_p2")
_ST = {}


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


def _strata(p, cfg, m):
    """The twin's pools, once per (data, membership, projection), shared read-only."""
    key = (id(p), cfg.n1p, cfg.n2p, bool(cfg.fold), int(cfg.ann_want), cfg.start_position, cfg.end_position, m)
    if key not in _ST:
        _ST[key] = PN.strata(p, cfg, *m)
    return _ST[key]


def _one_snp_plan(r, cfg):
    """A 1-SNP SNP-count-window plan on the run's device data, under the same membership; returns (plan, the record
    index of every SNP that is a window's only SNP, -1 elsewhere)."""
    c1 = _cfg(cfg.n1p, cfg.n2p, fold=cfg.fold, window_mode=L.WINDOW_SNPS, window=1, ann_want=cfg.ann_want,
              start_position=cfg.start_position, end_position=cfg.end_position)
    pl1 = r.pl.eng.plan(r.dev, c1)
    pl1.run()
    pl1.check()
    recs1 = pl1.read()
    of = np.full(r.p.n, -1, np.int64)
    live = np.nonzero(((recs1["flags"] & (L.W_EMPTY | L.W_EXTRA)) == 0) & (recs1["end"] - recs1["begin"] == 1))[0]
    of[recs1["begin"][live]] = live
    return pl1, of


def _check(p, r, cfg, m, R, seed=0, rec=None, what=""):
    """One project_null call of the plan of run ``r``, checked the three ways of the module docstring; returns
    (observed stats, null records, thin)."""
    pl = r.pl
    recs = pl.read()
    obs = pl.project_scan(*m)
    e, e_bg = pl.project_scan_e, pl.project_scan_e_bg
    null, thin = pl.project_null(*m, R, seed, rec)
    assert (pl.project_null_e, pl.project_null_e_bg) == (e, e_bg), what
    ent = list(range(len(recs))) if rec is None else [int(x) for x in rec]
    assert null.dtype == L.PROJSTAT_DTYPE and len(null) == len(ent) * R and len(thin) == len(ent)
    st = _strata(p, cfg, m)
    draws = PN.conditional_draws(p, recs, cfg, *m, ent, R, seed, st)
    # the twin's thin slots, n_used and n_dropped, the flags
    for t, s in enumerate(ent):
        fl = int(recs[s]["flags"]) & (L.W_EMPTY | L.W_EXTRA)
        blk = null[t * R:(t + 1) * R]
        if fl:
            assert (blk["flags"] == fl).all() and thin[t] == 0 and not any(blk[f].any() for f in blk.dtype.names if f != "flags")
            continue
        hi = min(int(recs[s]["end"]), p.n)
        lo = min(int(recs[s]["begin"]), hi)
        used = st.used[lo:hi]
        assert thin[t] == int((used & (st.size[lo:hi] < L.PNULL_THIN)).sum()), (what, s)
        assert (blk["n_used"] == obs["n_used"][s]).all() and (blk["n_dropped"] == obs["n_dropped"][s]).all(), (what, s)
        assert (blk["e"] == e).all() and not blk["flags"].any() and int(used.sum()) == int(obs["n_used"][s]), (what, s)
    # every replicate's grid from the device's own projection of the drawn SNPs
    pl1, of = _one_snp_plan(r, cfg)
    try:
        sel, grp = [], []
        for t, d in enumerate(draws):
            for k in range(R):
                g = d[k][d[k] >= 0] if d.shape[1] else d[k]
                sel.append(of[g])
                grp.append(np.full(len(g), t * R + k, np.int32))
        sel, grp = np.concatenate(sel), np.concatenate(grp)
        assert (sel >= 0).all(), what                                   # every drawn SNP is a 1-SNP window's
        grids, u, _ = pl1.project(*m, sel, grp, len(ent) * R)
        assert pl1.project_e == e, (what, pl1.project_e, e)              # the same rounding: the same exponent
        chroms = sorted({int(recs[s]["chrom"]) for s in ent})
        gb, _, _ = pl.project(*m, [-(c + 1) for c in chroms], np.arange(len(chroms), dtype=np.int32), len(chroms))
        assert pl.project_e == e_bg
    finally:
        pl1.close()
    worst = 0.0
    seen = {"finite": 0, "nan": 0, "inf": 0}
    for t, s in enumerate(ent):
        if int(recs[s]["flags"]) & (L.W_EMPTY | L.W_EXTRA):
            continue
        bgc = gb[chroms.index(int(recs[s]["chrom"]))]
        for k in range(R):
            q = null[t * R + k]
            g = grids[t * R + k]
            assert int(u[t * R + k]) == int(q["n_used"]), (what, s, k)
            assert (int(q["n2_fx"]), int(q["n1a_fx"]), int(q["n1b_fx"])) == PS.fixed_sums(g, cfg.fold, e), (what, s, k)
            for f, (T, A, _) in zip(FIELDS, PS.closed_form(g, bgc, cfg.fold)):
                got = float(q[f])
                if math.isnan(T) or math.isinf(T):
                    assert (math.isnan(got) and math.isnan(T)) or got == T, (what, s, k, f, got, T)
                    seen["nan" if math.isnan(T) else "inf"] += 1
                else:
                    assert math.isfinite(got) and abs(got - T) <= 1e-10 * A, (what, s, k, f, got, T, A)
                    seen["finite"] += 1
                    if A > 0:
                        worst = max(worst, abs(got - T) / A)
    print(f"{what}: {len(ent)} entries x {R}, e {e} / {e_bg}, worst err / A {worst:.3g}, {seen}, thin {int(thin.sum())}")
    return obs, null, thin


# ------------------------------------------------------------------------------------------- 1. shapes

@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
@pytest.mark.parametrize("m", [(2, 2), (7, 5), (24, 20)], ids=["2x2", "7x5", "24x20"])
def test_whole_chromosome_records(m, fold):
    """Records of 1, 63, 64, 65, 255, 256, 257, 2,047, 2,049 and 9,000 SNPs: below, at and above a wavefront row, a
    workgroup row and the rows in flight."""
    p = PS.genome(N1P, N2P, m)
    cfg = _cfg(fold=fold, regions=_whole_chroms(p))
    with SU.Run(p, cfg) as r:
        obs, null, thin = _check(p, r, cfg, m, 3, 5, None, f"whole chromosomes {m}")
        assert r.pl.project_null_e == 40
    assert (null["n_used"][::3] == obs["n_used"]).all() and obs["n_used"][-1] > 7000
    assert np.isfinite(null["t2d"][12:]).all() and (null["t2d"][12:] > -1e-9).all()


def test_windows_of_50():
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window_mode=L.WINDOW_SNPS, window=50)
    with SU.Run(p, cfg) as r:
        obs, null, thin = _check(p, r, cfg, M, 8, 1, None, "50-SNP windows")
    assert len(obs) > 250 and np.isfinite(null["t2d"]).all() and (null["t2d"] > 0).all()
    # the draws differ between replicates and between entries
    assert len(set(null["t2d"][:8].tolist())) == 8 and null["t2d"][:8].tolist() != null["t2d"][8:16].tolist()


def test_three_snp_windows_every_workgroup_walks_many():
    """About 4,700 entries x 2 on far fewer workgroups: a grid left over from the previous record would show; the
    all-dropped window is NaN in every replicate."""
    import torch
    m = (7, 5)
    p = PS.genome(N1P, N2P, m)
    cfg = _cfg(window_mode=L.WINDOW_SNPS, window=3)
    with SU.Run(p, cfg) as r:
        assert 2 * r.pl.nrec > 16 * torch.cuda.get_device_properties(0).multi_processor_count
        obs, null, thin = _check(p, r, cfg, m, 2, 0, None, "3-SNP windows")
        recs = r.pl.read()
    i = int(np.nonzero(recs["begin"] == int(p.chrom_off[-2]) + PS.ALL_DROPPED)[0][0])
    for k in range(2):
        q = null[2 * i + k]
        assert (q["n_used"], q["n_dropped"], q["n2_fx"]) == (0, 3, 0) and all(math.isnan(q[f]) for f in FIELDS)
    pv = PN.project_pvalues(obs, null, 2)
    assert math.isnan(pv["p_T2D_proj"][i]) and np.isfinite(pv["p_T2D_proj"]).sum() > 4000


def test_lds_opt_in_grid():
    """(160, 120) from 100 / 75: a 156 kB grid, above the default LDS limit; a few records."""
    n1p, n2p, m = 100, 75, (160, 120)
    p = PU.genome(n1p, n2p, m, lengths=[2049, 1000, 257])
    cfg = _cfg(n1p, n2p, regions=_whole_chroms(p))
    with SU.Run(p, cfg) as r:
        obs, null, thin = _check(p, r, cfg, m, 2, 0, [2, 1], "161 x 121")
        again, _ = r.pl.project_null(*m, 2, 0, [2, 1])
    assert null.tobytes() == again.tobytes() and null["n_used"].sum() > 1000 and np.isfinite(null["t2d"]).all()


# ------------------------------------------------------------------------------------------- 2. plan kinds

@pytest.mark.parametrize("fused", ["0", "1"], ids=["sliced", "fused"])
def test_tiled_plans(monkeypatch, fused):
    monkeypatch.setenv("SFS2D_FUSED", fused)
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window=20000, prev_extra=True)
    with SU.Run(p, cfg) as r:
        assert r.pl.scan_variant()["fused"] == int(fused) and r.pl.scan_variant()["cnt"] == 1
        obs, null, thin = _check(p, r, cfg, M, 2, 9, None, f"tiled fused={fused}")
    assert obs["flags"][-1] == L.W_EXTRA and (null["flags"][-2:] == L.W_EXTRA).all() and np.isfinite(null["t2d"]).sum() > 30


def test_sliding_plan():
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window=8000, step=2000)
    with SU.Run(p, cfg) as r:
        obs, null, _ = _check(p, r, cfg, M, 2, 0, None, "sliding")
    assert (obs["flags"] == 0).sum() > 50 and np.isfinite(null["t2d"]).sum() > 100


def test_regions_plan_with_an_empty_interval():
    from sfs2d.regions import Regions
    p = PS.genome(N1P, N2P, M)
    c8, c9 = p.chrom_names[8], p.chrom_names[9]
    items = [(c9, 10000, 200000, "outer"), (c9, 50000, 60000, "nested"), (c9, 1 << 30, 1 << 31, "empty"),
             (c8, 1, 1 << 31, "chrom8"), (c9, 50000, 60000, "nested_again")]
    rg = Regions(p.chrom_names, items)
    cfg = _cfg(regions=rg)
    with SU.Run(p, cfg) as r:
        obs, null, thin = _check(p, r, cfg, M, 3, 2, None, "regions")
    by = dict(zip(rg.slot_keys(), range(len(obs))))
    assert (null["flags"][3 * by["empty"]:3 * by["empty"] + 3] == L.W_EMPTY).all() and thin[by["empty"]] == 0
    # equal ranges at different record indices draw differently (the record index is in the counter)
    a, b = null[3 * by["nested"]:3 * by["nested"] + 3], null[3 * by["nested_again"]:3 * by["nested_again"] + 3]
    assert (a["n_used"] == b["n_used"]).all() and a["t2d"].tolist() != b["t2d"].tolist()


def test_attached_plans():
    p = PS.genome(N1P, N2P, M)
    base_cfg = _cfg(window=2000)
    cfgs = [_cfg(window=10000), _cfg(window_mode=L.WINDOW_SNPS, window=65)]
    with SU.Run(p, base_cfg, run=False) as r:
        att = [r.pl.attach(c) for c in cfgs]
        with pytest.raises(L.Sfs2dError) as ei:      # an attached plan has no records before its base runs
            att[0].project_null(*M, 2)
        assert ei.value.code == L.E_ARG
        r.pl.run()
        r.pl.check()

        class _R:      # (what _check reads of a run)
            pass
        for a, c in zip(att, cfgs):
            rr = _R()
            rr.pl, rr.dev, rr.p = a, r.dev, p
            _check(p, rr, c, M, 2, 0, None, f"attached {c.window_mode} {c.window}")


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
def test_filtered_plan_takes_the_bins(fold):
    """A position filter and variant_type: membership, and so the pools, from k_prep's stored bins word."""
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(fold=fold, window_mode=L.WINDOW_SNPS, window=513, **FILT)
    with SU.Run(p, cfg) as r:
        assert r.pl.scan_variant()["cnt"] == 0
        obs, null, _ = _check(p, r, cfg, M, 2, 0, None, "filtered")
    free = _strata(p, _cfg(fold=fold), M)
    assert 0 < obs["n_used"].sum() < free.used.sum() / 2


def test_wrapped_device_data():
    import wide_util as WU
    from sfs2d.engine import Engine
    p = PS.genome(N1P, N2P, M)
    for filt, ann in (({}, False), (FILT, True)):
        d, keep = WU.wrapped(Engine.get(0), p, ann=ann)
        try:
            cfg = _cfg(window=20000, **filt)
            with SU.Run(p, cfg, dev=d) as r:
                _check(p, r, cfg, M, 2, 0, None, f"wrapped {filt}")
        finally:
            d.close()
        del keep


# ------------------------------------------------------------------------------------------- 3. contract

def test_determinism_split_and_order():
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window_mode=L.WINDOW_SNPS, window=50)
    R = 4
    with SU.Run(p, cfg) as r:
        a, ta = r.pl.project_null(*M, R, 3)
        b, tb = r.pl.project_null(*M, R, 3)
        r.pl.project_null(7, 5, 2, 3, [0, 1])                 # another projection in between: the pools are rebuilt
        r.pl.project_scan(7, 5)
        c, tc = r.pl.project_null(*M, R, 3)
        assert a.tobytes() == b.tobytes() == c.tobytes() and ta.tobytes() == tb.tobytes() == tc.tobytes()
        n = len(ta)
        lo, tl = r.pl.project_null(*M, R, 3, list(range(100)))
        hi, th = r.pl.project_null(*M, R, 3, list(range(100, n)))
        assert lo.tobytes() + hi.tobytes() == a.tobytes() and tl.tobytes() + th.tobytes() == ta.tobytes()
        order = np.random.default_rng(0).permutation(n)
        sh, ts = r.pl.project_null(*M, R, 3, order)
        assert np.array_equal(sh.reshape(n, R)[np.argsort(order)].reshape(-1), a) and np.array_equal(ts[np.argsort(order)], ta)
        other, _ = r.pl.project_null(*M, R, 4)
        assert other.tobytes() != a.tobytes() and np.array_equal(other["n_used"], a["n_used"])


@pytest.mark.parametrize("fused", ["0", "1"], ids=["sliced", "fused"])
def test_following_runs_and_other_reads_are_untouched(monkeypatch, fused):
    """run, project_null, run (both replica parities) leaves the later runs' records and Fst, and the null, diversity,
    spectra, project and project_scan reads, byte-equal to a plan that never called it."""
    monkeypatch.setenv("SFS2D_FUSED", fused)
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window=5000, fst=True, prev_extra=True)
    with SU.Run(p, cfg) as ref:
        want = []
        for _ in range(2):
            ref.pl.run()
            ref.pl.check()
            want.append((ref.pl.read().tobytes(), ref.pl.read_fst().tobytes()))
        div, spec = ref.pl.diversity().tobytes(), ref.pl.spectra().tobytes()
        proj = [x.tobytes() for x in ref.pl.project(*M)]
        pscan = ref.pl.project_scan(*M).tobytes()
        ref.pl.null_run([(0, 1), (9, 513)], 8, 3)
        null = ref.pl.null_read().tobytes()
    with SU.Run(p, cfg) as r:
        first = None
        for k in range(2):
            ps = r.pl.project_scan(*M)
            got = r.pl.project(*M)
            s, t = r.pl.project_null(*M, 3, 1)
            r.pl.project_null(7, 5, 2, 1, [0, 3])
            assert ps.tobytes() == pscan
            out = np.zeros(len(ps), L.PROJSTAT_DTYPE)      # project_scan_read of the earlier call
            n, w = C.c_int64(), C.c_int64()
            assert r.pl.eng.lib.sfs2d_plan_project_scan_read(r.pl.h, L.ptr(out), len(out), C.byref(n)) == 0
            assert out.tobytes() == pscan
            o2, uu, dd = np.zeros_like(got[0]), np.zeros_like(got[1]), np.zeros_like(got[2])
            assert r.pl.eng.lib.sfs2d_plan_project_read(r.pl.h, L.ptr(o2), L.ptr(uu), L.ptr(dd), len(o2), C.byref(n),
                                                        C.byref(w)) == 0 and o2.tobytes() == proj[0]
            assert r.pl.spectra().tobytes() == spec and r.pl.diversity().tobytes() == div
            assert [x.tobytes() for x in r.pl.project(*M)] == proj
            r.pl.null_run([(0, 1), (9, 513)], 8, 3)
            assert r.pl.null_read().tobytes() == null
            s2, t2 = r.pl.project_null(*M, 3, 1)
            assert s.tobytes() == s2.tobytes() and t.tobytes() == t2.tobytes()
            first = s if first is None else first
            assert s.tobytes() == first.tobytes()      # every run alike
            r.pl.run()
            r.pl.check()
            assert (r.pl.read().tobytes(), r.pl.read_fst().tobytes()) == want[k], k


def test_caller_buffers():
    import torch
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window=20000)
    R = 3
    with SU.Run(p, cfg) as r:
        st, thin = r.pl.project_null(*M, R, 2)
        n = len(thin)
        buf = torch.full((n * R * 8 + 8,), 7, dtype=torch.int64, device="cuda:0")
        tb = torch.full((n + 4,), 9, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        none, thin2 = r.pl.project_null(*M, R, 2, out_dev_ptr=buf.data_ptr())
        r.pl.check()
        got = buf.cpu().numpy()
        assert none is None and np.array_equal(thin2, thin)
        assert (got[n * R * 8:] == 7).all() and got[:n * R * 8].tobytes() == st.tobytes()
        # the device p-values from the caller's buffer equal the host's
        obs = r.pl.project_scan(*M)
        pv = PN.project_pvalues(obs, st, R)
        pd = PN.project_pvalues_device(obs, buf[:n * R * 8].view(torch.uint8), R)
        assert all(np.array_equal(pv[k], pd[k], equal_nan=True) for k in PN.PROJ_P_KEYS) and np.isfinite(pv["p_T2D_proj"]).sum() > 15
        # both outputs in the caller's buffers through the C call
        npar = L.NullParams(seed=2, replicates=R)
        buf.fill_(7)
        torch.cuda.synchronize()
        assert r.pl.eng.lib.sfs2d_plan_project_null(r.pl.h, *M, C.byref(npar), None, n, C.c_void_p(buf.data_ptr()),
                                                    C.c_void_p(tb.data_ptr()), None, None) == 0
        r.pl.check()
        assert buf.cpu().numpy()[:n * R * 8].tobytes() == st.tobytes()
        assert np.array_equal(tb.cpu().numpy()[:n].astype(np.uint32), thin) and (tb.cpu().numpy()[n:] == 9).all()
        # the read call copies from where the last call wrote
        out, th = np.zeros(n * R, L.PROJSTAT_DTYPE), np.zeros(n, np.uint32)
        k = C.c_int64()
        assert r.pl.eng.lib.sfs2d_plan_project_null_read(r.pl.h, L.ptr(out), L.ptr(th), n * R, C.byref(k)) == 0
        assert k.value == n * R and out.tobytes() == st.tobytes() and np.array_equal(th, thin)


def test_refusals():
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window=20000)
    with SU.Run(p, cfg, run=False) as r:
        lib, h, nrec = r.pl.eng.lib, r.pl.h, r.pl.nrec
        err = lambda: lib.sfs2d_last_error(r.pl.eng.h).decode()
        n, e, eb = C.c_int64(), C.c_int32(), C.c_int32()
        R = 2
        out, th = np.zeros(nrec * R, L.PROJSTAT_DTYPE), np.zeros(nrec, np.uint32)

        def call(m1, m2, rec=None, reps=R, nsel=None):
            npar = L.NullParams(seed=0, replicates=reps)
            a = None if rec is None else np.ascontiguousarray(np.asarray(rec, np.int64))
            return lib.sfs2d_plan_project_null(h, m1, m2, C.byref(npar), None if a is None else C.c_void_p(a.ctypes.data),
                                               (nrec if a is None else len(a)) if nsel is None else nsel, None, None,
                                               C.byref(e), C.byref(eb))
        read = lambda cap: lib.sfs2d_plan_project_null_read(h, L.ptr(out), L.ptr(th), cap, C.byref(n))
        assert call(24, 20) == L.E_ARG and "first run" in err()                                # a plan that has not run
        assert read(nrec * R) == L.E_ARG and "before sfs2d_plan_project_null" in err()         # no call yet
        r.pl.run()
        r.pl.check()
        for m1, m2 in ((1, 20), (37, 20), (24, 1), (24, 29), (0, 0), (-3, 20)):
            assert call(m1, m2) == L.E_ARG and "outside [2, 36] x [2, 28]" in err(), (m1, m2)
        assert call(24, 20, reps=0) == L.E_ARG and "replicates" in err()
        for bad in ([-1], [nrec], [0, 1 << 40]):
            assert call(24, 20, bad) == L.E_ARG and "record" in err(), bad
        assert call(24, 20, nsel=nrec - 1) == L.E_ARG and "nsel" in err()                      # rec == NULL: every record
        assert lib.sfs2d_plan_project_null(h, 24, 20, None, None, nrec, None, None, None, None) == L.E_ARG
        assert read(nrec * R) == L.E_ARG                                                       # still none
        assert call(24, 20, reps=(1 << 26) // nrec + 1) == L.E_CAP and "2^26" in err()
        assert call(24, 20) == 0 and (e.value, eb.value) == (40, 40)
        assert read(nrec * R - 1) == L.E_CAP and n.value == nrec * R                           # a short read buffer
        assert read(nrec * R) == 0 and np.isfinite(out["t2d"]).sum() > 30
        assert call(24, 20, []) == 0 and read(0) == 0 and n.value == 0                         # an empty selection
    # a plan with a supplied background
    cfg = _cfg(window=20000, bg_mode=L.BG_SUPPLIED)
    bg = (np.ones((2 * N1P + 1) * (2 * N2P + 1)), np.ones(N1P + 1), np.ones(N2P + 1))
    with SU.Run(p, cfg, bg=bg) as r:
        with pytest.raises(L.Sfs2dError) as ei:
            r.pl.project_null(*M, 2)
        assert ei.value.code == L.E_ARG and "supplied background" in str(ei.value)
    # a grid beyond the LDS
    pb = PU.genome(127, 127, (254, 254), lengths=[257], full=True)
    cfg = _cfg(127, 127, regions=_whole_chroms(pb))
    with SU.Run(pb, cfg) as r:
        with pytest.raises(L.Sfs2dError) as ei:
            r.pl.project_null(254, 254, 2)
        assert ei.value.code == L.E_CAP and "LDS" in str(ei.value)


def test_exponents_are_the_projected_scans():
    """Both calls take e and e_bg from one host helper (its e < 8 refusal needs a record bound above 2^54 SNPs, which
    32-bit SNP indices cannot reach: not provoked here)."""
    p = PS.genome(N1P, N2P, M)
    cfg = _cfg(window=20000)
    with SU.Run(p, cfg) as r:
        r.pl.project_scan(*M)
        r.pl.project_null(*M, 1, 0, [0])
        assert (r.pl.project_null_e, r.pl.project_null_e_bg) == (r.pl.project_scan_e, r.pl.project_scan_e_bg)


# ------------------------------------------------------------------------------------------- 4. class and CLI

def test_class_projected_scan_with_replicates():
    import twoDSFS_class as T
    p = PS.genome(N1P, N2P, M)
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=N1P, pop2_size=N2P)
    R = 9
    for kw, ckw, kind in (({"window_size": 20000}, {"window": 20000}, "bp"),
                          ({"snp_window_size": 257}, {"window_mode": L.WINDOW_SNPS, "window": 257}, "snps")):
        cfg = _cfg(**ckw)
        with SU.Run(p, cfg) as r:
            recs = r.pl.read()
            st = r.pl.project_scan(*M)
            null, thin = r.pl.project_null(*M, R, 5)
        labels = post.record_labels(recs, p, kind, ckw["window"], None)
        want = PN.add_pvalue_columns(SP.project_scan_rows(recs, st, labels), labels, PN.project_pvalues(st, null, R), thin)
        plain = obj.projected_scan(p, M, **kw)
        got = obj.projected_scan(p, M, replicates=R, seed=5, **kw)
        assert got == want and list(got) == list(want) and len(got) > 20
        assert {k: {c: v[c] for c in SP.PROJSCAN_COLUMNS} for k, v in got.items()} == plain      # the old columns as they were
        assert all(list(v)[-7:] == PN.PROJNULL_COLUMNS for v in got.values())
        ps = [v["p_T2D_proj"] for v in got.values() if v["p_T2D_proj"] is not None]
        assert len(ps) > 15 and all(1 / (R + 1) <= x <= 1 for x in ps)
    items = [(p.chrom_names[9], 10000, 200000, "outer"), (p.chrom_names[9], 1 << 30, 1 << 31, "empty"),
             (p.chrom_names[8], 1, 1 << 31, "chrom8")]
    got = obj.projected_scan(p, M, regions=items, replicates=R)
    assert list(got) == ["outer", "empty", "chrom8"] and got["empty"]["p_T2D_proj"] is None and got["empty"]["n_thin"] == 0
    assert got["outer"]["p_T2D_proj"] is not None and got["chrom8"]["n_thin"] > 0


def test_fixed_differences_window_is_the_most_extreme():
    """A window overwritten with fixed differences (every SNP fixed for alt in population 1, for ref in population 2,
    fully called): no replicate of its own strata reaches its T2D, p = 1 / (R + 1)."""
    import twoDSFS_class as T
    from sfs2d.pack import PackedSNPs, pack_counts
    p = PS.genome(N1P, N2P, M)
    cols = [p.ref1.astype(np.int64), p.alt1.astype(np.int64), p.ref2.astype(np.int64), p.alt2.astype(np.int64)]
    lo = int(p.chrom_off[9]) + 50 * 40
    for f, v in zip(cols, (0, 2 * N1P, 2 * N2P, 0)):
        f[lo:lo + 50] = v
    q = PackedSNPs(pack_counts(*cols), p.pos, p.chrom_off, p.chrom_names, p.ann_id, p.ann_names)
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=N1P, pop2_size=N2P, fold=False)
    R = 19
    got = obj.projected_scan(q, M, snp_window_size=50, replicates=R)
    rows = [v for k, v in got.items() if k.startswith(p.chrom_names[9] + " ")]
    hit = max(rows, key=lambda v: -1.0 if v["T2D_proj"] is None else v["T2D_proj"])
    assert hit["n_used"] == 50 and hit["p_T2D_proj"] == 1 / (R + 1)
    assert sum(v["p_T2D_proj"] == 1 / (R + 1) for v in rows) < len(rows) / 4


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
    bed.write_text(f"{c0}\t{int(P0[10]) - 1}\t{int(P0[60])}\tgeneA\n{c0}\t{int(P0[-1]) + 10}\t{int(P0[-1]) + 20}\tempty\n")
    base = [vcf, pm, "--pop1", "uv", "--pop2", "bv", "--pop1-size", "11", "--pop2-size", "11", "--window", "500000",
            "--snp-window", "100", "--regions", str(bed), "--project-scan", "16,14"]
    plain = cli.main(base + ["--out-prefix", str(tmp_path / "p")])
    capsys.readouterr()
    outs = cli.main(base + ["--project-null", "9", "--null-seed", "4", "--out-prefix", str(tmp_path / "s")])
    errtext = capsys.readouterr().err
    assert sorted(os.path.basename(x)[1:] for x in outs) == sorted(os.path.basename(x)[1:] for x in plain)
    assert errtext.count("used slots are thin") == 3 and "project_null R = 9" in errtext
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=11, pop2_size=11)
    for a in plain:
        b = str(tmp_path / ("s" + os.path.basename(a)[1:]))
        if "_projscan" not in a:      # every other file is what it was
            assert _read(a) == _read(b)
            continue
        with open(a, newline="") as fa, open(b, newline="") as fb:
            ra, rb = list(csv.DictReader(fa)), list(csv.DictReader(fb))
        assert list(rb[0]) == list(ra[0]) + PN.PROJNULL_COLUMNS and len(ra) == len(rb)
        assert all({k: y[k] for k in x} == x for x, y in zip(ra, rb))      # the old columns as they were
    for stem, kw in (("s_500kb", {"window_size": 500000}), ("s_100snps", {"snp_window_size": 100}),
                     ("s_regions", {"regions": str(bed)})):
        want = obj.projected_scan(p, (16, 14), replicates=9, seed=4, **kw)
        with open(tmp_path / (stem + "_projscan16x14.csv"), newline="") as fh:
            rows = list(csv.DictReader(fh))
        for row, (lb, w) in zip(rows, want.items()):
            for k in PN.PROJNULL_COLUMNS:
                assert row[k] == ("" if w[k] is None else str(w[k])), (stem, lb, k)
    assert want["empty"]["p_T2D_proj"] is None and want["geneA"]["p_T2D_proj"] is not None
