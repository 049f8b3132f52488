"""The refusals of the nine post-scan entry points -- null run / read, diversity / read, spectra / read, project /
read, project_scan / read -- pinned as (return code, sfs2d_last_error text) to tests/golden/postscan_refusals.json,
which was recorded once with this table from the build before the calls came to share their plumbing (DESIGN.md,
"post-scan calls: the common skeleton").  ``python tests/test_postscan_refusals_gpu.py`` records the file.

The fixture is project_util.genome at 18 / 14: two chromosomes of 40,000 and 30,000 SNPs around an empty one (the
null's "pool is empty"), 20 kb windows, ~200 records.  Three plans: ``pl`` (per-chromosome backgrounds), ``att``
attached to it at 40 kb (the null's refusal of attached plans, and the other calls' words for an attached plan whose
base has not run) and ``sup`` (a supplied background).  The table is a sequence: the plans run partway through it.
It holds every refusal that test_refusals of the null, block-null, diversity, spectra, project and projected-scan
tests reach, the successful calls between them (code 0, no text), and the two-fault cases of spectra and project:
a bad entry together with rows that do not fit 64 bits, which spectra blames on the entry and project on the rows.
Texts that never reach a device are compared; the data set above 2^32 - 1 SNPs is not reachable here."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N1P, N2P, M1, M2 = 18, 14, 24, 20
LENGTHS = [40000, 0, 30000]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postscan_refusals.json")


def _i64(*v):
    return np.array(v, np.int64)


def _i32(*v):
    return np.array(v, np.int32)


def outcomes():
    """[[label, return code, error text ("" on success)], ...] of the table, in order."""
    import project_util as PU
    from sfs2d import _lib as L
    from sfs2d.engine import Engine, ScanConfig

    p = PU.genome(N1P, N2P, None, lengths=LENGTHS)
    eng = Engine.get(0)
    lib = eng.lib
    dev = eng.upload(p)
    pl = eng.plan(dev, ScanConfig(n1p=N1P, n2p=N2P, window=20000, bg_mode=L.BG_PER_CHROM))
    att = pl.attach(ScanConfig(n1p=N1P, n2p=N2P, window=40000, bg_mode=L.BG_PER_CHROM))
    sup = eng.plan(dev, ScanConfig(n1p=N1P, n2p=N2P, window=20000, bg_mode=L.BG_SUPPLIED))
    sup.set_background(np.ones((2 * N1P + 1) * (2 * N2P + 1)), np.ones(N1P + 1), np.ones(N2P + 1))
    nrec, nchrom = pl.nrec, p.nchrom
    assert nchrom == 3 and 100 <= nrec <= 400, (nchrom, nrec)
    out = []
    n, w, e, eb = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
    keep = []   # (the argument arrays of a call stay alive until it returns)

    def ptr(a):
        keep.append(a)
        return None if a is None else C.c_void_p(a.ctypes.data)

    def null(h, tasks, reps=3, block=None, seed=11):
        npar = L.NullParams(seed=seed, replicates=reps)
        t = None if tasks is None else np.asarray(tasks, np.int64).reshape(-1, 2)
        nt = 0 if t is None else len(t)
        if block is None:
            return lib.sfs2d_plan_null_run(h, C.byref(npar), ptr(t), nt, None)
        return lib.sfs2d_plan_null_run_blocks(h, C.byref(npar), block, ptr(t), nt, None)

    wbuf = np.zeros(1 << 16, L.WINDOW_DTYPE)
    dbuf = np.zeros(nrec, L.DIVERSITY_DTYPE)
    sbuf = np.zeros(nrec * L.spec_row_words(N1P, N2P), np.int64)
    pg, pu, pd = np.zeros((nrec, M1 + 1, M2 + 1)), np.zeros(nrec, np.int64), np.zeros(nrec, np.int64)
    qbuf = np.zeros(nrec, L.PROJSTAT_DTYPE)

    def null_read(h, cap):
        return lib.sfs2d_plan_null_read(h, ptr(wbuf), cap, C.byref(n))

    def div(h):
        return lib.sfs2d_plan_diversity(h, None)

    def div_read(h, cap):
        return lib.sfs2d_plan_diversity_read(h, ptr(dbuf), cap, C.byref(n))

    def spec(h, rec, grp, nsel, ng):
        return lib.sfs2d_plan_spectra(h, ptr(rec), ptr(grp), nsel, ng, None)

    def spec_read(h, cap):
        return lib.sfs2d_plan_spectra_read(h, ptr(sbuf), cap, C.byref(n))

    def proj(h, m1, m2, rec, grp, nsel, ng):
        return lib.sfs2d_plan_project(h, m1, m2, ptr(rec), ptr(grp), nsel, ng, None, C.byref(e))

    def proj_read(h, cap):
        return lib.sfs2d_plan_project_read(h, ptr(pg), ptr(pu), ptr(pd), cap, C.byref(n), C.byref(w))

    def pscan(h, m1, m2, bg):
        return lib.sfs2d_plan_project_scan(h, m1, m2, bg, None, C.byref(e), C.byref(eb))

    def pscan_read(h, cap):
        return lib.sfs2d_plan_project_scan_read(h, ptr(qbuf), cap, C.byref(n))

    a, g = _i64(0, 1), _i32(0, 0)
    BIG = 1 << 62
    table = [
        # ---- before any run
        ("null: plan not run", lambda: null(pl.h, [(0, 5)])),
        ("null blocks: plan not run", lambda: null(pl.h, [(0, 5)], block=4)),
        ("null: supplied plan not run", lambda: null(sup.h, [(-1, 5)])),
        ("null: attached, not run", lambda: null(att.h, [(0, 5)])),
        ("null read: no call yet", lambda: null_read(pl.h, 0)),
        ("diversity: plan not run", lambda: div(pl.h)),
        ("diversity: attached, base not run", lambda: div(att.h)),
        ("diversity read: no call yet", lambda: div_read(pl.h, nrec)),
        ("spectra: plan not run", lambda: spec(pl.h, None, None, nrec, nrec)),
        ("spectra: attached, base not run", lambda: spec(att.h, None, None, att.nrec, att.nrec)),
        ("spectra read: no call yet", lambda: spec_read(pl.h, sbuf.size)),
        ("project: plan not run", lambda: proj(pl.h, M1, M2, None, None, nrec, nrec)),
        ("project: attached, base not run", lambda: proj(att.h, M1, M2, None, None, att.nrec, att.nrec)),
        ("project read: no call yet", lambda: proj_read(pl.h, nrec)),
        ("project_scan: plan not run", lambda: pscan(pl.h, M1, M2, -1)),
        ("project_scan: attached, base not run", lambda: pscan(att.h, M1, M2, -1)),
        ("project_scan read: no call yet", lambda: pscan_read(pl.h, nrec)),
        # ---- the plans run
        ("run pl", lambda: (pl.run(), pl.check(), 0)[2]),
        ("run sup", lambda: (sup.run(), sup.check(), 0)[2]),
        # ---- null
        ("null: null params", lambda: lib.sfs2d_plan_null_run(pl.h, None, ptr(_i64(0, 5)), 1, None)),
        ("null: ntasks < 0", lambda: lib.sfs2d_plan_null_run(pl.h, C.byref(L.NullParams(seed=1, replicates=3)), None, -1, None)),
        ("null: tasks NULL", lambda: lib.sfs2d_plan_null_run(pl.h, C.byref(L.NullParams(seed=1, replicates=3)), None, 1, None)),
        ("null: attached plan", lambda: null(att.h, [(0, 5)])),
        ("null: pool past the end", lambda: null(pl.h, [(0, 5), (3, 5)])),
        ("null: pool -2", lambda: null(pl.h, [(-2, 5)])),
        ("null: pool -1 per chromosome", lambda: null(pl.h, [(-1, 5)])),
        ("null: empty pool", lambda: null(pl.h, [(1, 5)])),
        ("null: m 0", lambda: null(pl.h, [(0, 0)])),
        ("null: m -3", lambda: null(pl.h, [(0, -3)])),
        ("null: m 2^32", lambda: null(pl.h, [(0, 1 << 32)])),
        ("null: replicates 0", lambda: null(pl.h, [(0, 5)], reps=0)),
        ("null: 2^27 records", lambda: null(pl.h, [(0, 5)], reps=1 << 27)),
        ("null blocks: block 0", lambda: null(pl.h, [(0, 5)], block=0)),
        ("null blocks: block -1", lambda: null(pl.h, [(0, 5)], block=-1)),
        ("null blocks: block 2^32", lambda: null(pl.h, [(0, 5)], block=1 << 32)),
        ("null blocks: pool -1", lambda: null(pl.h, [(-1, 5)], block=4)),
        ("null blocks: empty pool", lambda: null(pl.h, [(1, 5)], block=4)),
        ("null blocks: m 0", lambda: null(pl.h, [(0, 0)], block=4)),
        ("null blocks: replicates 0", lambda: null(pl.h, [(0, 5)], reps=0, block=4)),
        ("null blocks: attached plan", lambda: null(att.h, [(0, 5)], block=4)),
        ("null: supplied, empty pool", lambda: null(sup.h, [(1, 5)])),
        ("null: supplied, pool -1 is fine", lambda: null(sup.h, [(-1, 5)])),
        ("null: good call", lambda: null(pl.h, [(0, 5), (2, 6)])),
        ("null read: capacity", lambda: null_read(pl.h, 5)),
        ("null read: NULL buffer", lambda: lib.sfs2d_plan_null_read(pl.h, None, 6, C.byref(n))),
        ("null read: good", lambda: null_read(pl.h, 6)),
        ("null blocks: longest block", lambda: null(pl.h, [(0, 5), (2, 6)], block=(1 << 32) - 1)),
        # ---- diversity
        ("diversity read: still none", lambda: div_read(pl.h, nrec)),
        ("diversity: good call", lambda: div(pl.h)),
        ("diversity read: capacity", lambda: div_read(pl.h, nrec - 1)),
        ("diversity read: NULL buffer", lambda: lib.sfs2d_plan_diversity_read(pl.h, None, nrec, C.byref(n))),
        ("diversity read: good", lambda: div_read(pl.h, nrec)),
        # ---- spectra
        ("spectra: nsel -1", lambda: spec(pl.h, a, g, -1, 1)),
        ("spectra: ngroups 0", lambda: spec(pl.h, a, g, 2, 0)),
        ("spectra: record nrec", lambda: spec(pl.h, _i64(0, nrec), g, 2, 1)),
        ("spectra: record -1", lambda: spec(pl.h, _i64(-1, 0), g, 2, 1)),
        ("spectra: group 1 of 1", lambda: spec(pl.h, a, _i32(0, 1), 2, 1)),
        ("spectra: group -1", lambda: spec(pl.h, a, _i32(-1, 0), 2, 1)),
        ("spectra: bad record and bad group in one entry", lambda: spec(pl.h, _i64(nrec, 0), _i32(5, 0), 2, 1)),
        ("spectra: rec without grp", lambda: spec(pl.h, a, None, 2, 2)),
        ("spectra: NULL rec, nsel nrec - 1", lambda: spec(pl.h, None, None, nrec - 1, nrec)),
        ("spectra: NULL grp, ngroups nrec - 1", lambda: spec(pl.h, None, None, nrec, nrec - 1)),
        ("spectra: 2^62 rows", lambda: spec(pl.h, a, g, 2, BIG)),
        ("spectra: 2^31 rows", lambda: spec(pl.h, a, g, 2, 1 << 31)),
        ("spectra: bad record and 2^62 rows", lambda: spec(pl.h, _i64(0, nrec), g, 2, BIG)),
        ("spectra: bad group and 2^62 rows", lambda: spec(pl.h, a, _i32(0, -1), 2, BIG)),
        ("spectra read: still none", lambda: spec_read(pl.h, sbuf.size)),
        ("spectra: good call", lambda: spec(pl.h, None, None, nrec, nrec)),
        ("spectra read: capacity", lambda: spec_read(pl.h, sbuf.size - 1)),
        ("spectra read: NULL buffer", lambda: lib.sfs2d_plan_spectra_read(pl.h, None, sbuf.size, C.byref(n))),
        ("spectra read: good", lambda: spec_read(pl.h, sbuf.size)),
        # ---- project
        *[(f"project: m ({m1}, {m2})", lambda m1=m1, m2=m2: proj(pl.h, m1, m2, a, g, 2, 1))
          for m1, m2 in ((1, 20), (37, 20), (24, 1), (24, 29), (0, 0), (-3, 20))],
        ("project: nsel -1", lambda: proj(pl.h, M1, M2, a, g, -1, 1)),
        ("project: ngroups 0", lambda: proj(pl.h, M1, M2, a, g, 2, 0)),
        ("project: record nrec", lambda: proj(pl.h, M1, M2, _i64(0, nrec), g, 2, 1)),
        ("project: chromosome past the end", lambda: proj(pl.h, M1, M2, _i64(0, -(nchrom + 1)), g, 2, 1)),
        ("project: chromosome 2^40", lambda: proj(pl.h, M1, M2, _i64(-(1 << 40), 0), g, 2, 1)),
        ("project: group 1 of 1", lambda: proj(pl.h, M1, M2, a, _i32(0, 1), 2, 1)),
        ("project: group -1", lambda: proj(pl.h, M1, M2, a, _i32(-1, 0), 2, 1)),
        ("project: bad record and bad group in one entry", lambda: proj(pl.h, M1, M2, _i64(nrec, 0), _i32(5, 0), 2, 1)),
        ("project: bad chromosome and bad group in one entry", lambda: proj(pl.h, M1, M2, _i64(-9, 0), _i32(5, 0), 2, 1)),
        ("project: rec without grp", lambda: proj(pl.h, M1, M2, a, None, 2, 2)),
        ("project: NULL rec, nsel nrec - 1", lambda: proj(pl.h, M1, M2, None, None, nrec - 1, nrec)),
        ("project: NULL grp, ngroups nrec - 1", lambda: proj(pl.h, M1, M2, None, None, nrec, nrec - 1)),
        ("project: 2^62 rows", lambda: proj(pl.h, M1, M2, a, g, 2, BIG)),
        ("project: 2^31 rows", lambda: proj(pl.h, M1, M2, a, g, 2, 1 << 31)),
        ("project: bad record and 2^62 rows", lambda: proj(pl.h, M1, M2, _i64(0, nrec), g, 2, BIG)),
        ("project: bad group and 2^62 rows", lambda: proj(pl.h, M1, M2, a, _i32(0, -1), 2, BIG)),
        ("project read: still none", lambda: proj_read(pl.h, nrec)),
        ("project: good call", lambda: proj(pl.h, M1, M2, _i64(0, -nchrom), _i32(0, 1), 2, nrec)),
        ("project read: capacity", lambda: proj_read(pl.h, nrec - 1)),
        ("project read: NULL buffers", lambda: lib.sfs2d_plan_project_read(pl.h, None, None, None, nrec, C.byref(n), C.byref(w))),
        ("project read: good", lambda: proj_read(pl.h, nrec)),
        # ---- project_scan
        *[(f"project_scan: m ({m1}, {m2})", lambda m1=m1, m2=m2: pscan(pl.h, m1, m2, -1))
          for m1, m2 in ((1, 20), (37, 20), (24, 1), (24, 29), (0, 0), (-3, 20))],
        *[(f"project_scan: bg_chrom {bg}", lambda bg=bg: pscan(pl.h, M1, M2, bg)) for bg in (-2, nchrom, 1 << 20)],
        ("project_scan: supplied background", lambda: pscan(sup.h, M1, M2, -1)),
        ("project_scan read: still none", lambda: pscan_read(pl.h, nrec)),
        ("project_scan: good call, one chromosome", lambda: pscan(pl.h, M1, M2, nchrom - 1)),
        ("project_scan: good call, no exponents", lambda: lib.sfs2d_plan_project_scan(pl.h, M1, M2, -1, None, None, None)),
        ("project_scan read: capacity", lambda: pscan_read(pl.h, nrec - 1)),
        ("project_scan read: NULL buffer", lambda: lib.sfs2d_plan_project_scan_read(pl.h, None, nrec, C.byref(n))),
        ("project_scan read: good", lambda: pscan_read(pl.h, nrec)),
        # ---- an attached plan after its base has run serves the four calls
        ("diversity: attached plan", lambda: div(att.h)),
        ("spectra: attached plan", lambda: spec(att.h, None, None, att.nrec, att.nrec)),
    ]
    try:
        for label, call in table:
            rc = int(call())
            out.append([label, rc, lib.sfs2d_last_error(eng.h).decode() if rc else ""])
            keep.clear()
        pl.check()
    finally:
        pl.close()
        sup.close()
        dev.close()
    assert len({o[0] for o in out}) == len(out)   # (labels are the golden file's keys)
    return out


def test_refusals_are_the_recorded_ones():
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = outcomes()
    assert [o[0] for o in got] == [o[0] for o in want]
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, diff[:5]
    codes = {o[1] for o in got}
    assert {0, -1, -3, -6} <= codes                       # OK, E_ARG, E_NOMEM, E_CAP all occur
    assert sum(1 for o in got if o[1]) >= 80


if __name__ == "__main__":
    import sys
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(REPO, "2dsfs-scan_amd"), REPO, os.path.join(REPO, "tests")]
    dst = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    res = outcomes()
    with open(dst, "w") as fh:
        json.dump(res, fh, indent=0)
        fh.write("\n")
    print("recorded", len(res), "outcomes,", sum(1 for o in res if o[1]), "refusals ->", dst)
