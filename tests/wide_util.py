"""Helpers of the 32-bit-bin and position-edge tests (test_wide_bins.py, test_position_edges.py) and the record
check test_scan_variants.py shares with them.

``wrapped`` hands a data set over as sfs2d_data_wrap_device does: device arrays the caller owns, no host copy of
the positions -- the route on which plan_create cannot bound a window's SNPs and takes 32-bit 2D bins for every
fixed-bp window above 65,535 bp and every sliding plan.  ``check_records`` / ``check_against_oracle`` compare a
record table and its Fst column with the oracle window by window."""
import math

import numpy as np

import golden_util as gu
from oracle import sfs_oracle as O

INTS = ("chrom", "wid", "begin", "end", "snp_count", "n2", "n2_all", "n1a", "n1b", "flags")
_REF = {}


def wrapped(eng, p, ann=False):
    """(DeviceData of eng.wrap_device, the torch tensors it reads): p.counts / p.pos (p.ann_id with ``ann``)
    copied into device tensors padded by 64 elements.  The caller keeps the tensors alive until it has closed
    the data."""
    import torch
    dev = torch.device(f"cuda:{eng.device}")

    def up(a, view, dt):
        t = torch.zeros(len(a) + 64, dtype=dt, device=dev)
        if len(a):
            t[: len(a)].copy_(torch.from_numpy(np.ascontiguousarray(a).view(view)))
        return t

    counts = up(p.counts, np.int32, torch.int32)
    pos = up(p.pos, np.int32, torch.int32)
    annt = up(p.ann_id, np.int16, torch.int16) if ann else None
    torch.cuda.synchronize()   # the library reads the arrays on its own stream
    last = np.array([int(p.pos[int(p.chrom_off[c + 1]) - 1]) if p.chrom_off[c + 1] > p.chrom_off[c] else 0
                     for c in range(p.nchrom)], np.uint32)
    d = eng.wrap_device(counts.data_ptr(), pos.data_ptr(), annt.data_ptr() if ann else None, p.n, p.chrom_off, last)
    return d, (counts, pos, annt)


def run_plan(data, cfg, bg=None):
    """One plan of ``cfg`` on ``data`` run once: (records, Fst or None, Plan.scan_variant()); the plan is closed."""
    pl = data.eng.plan(data, cfg)
    try:
        if bg is not None:
            pl.set_background(*bg)
        pl.run()
        pl.check()
        return pl.read(), (pl.read_fst() if cfg.fst else None), pl.scan_variant()
    finally:
        pl.close()


def sliding_slots(p, w, s):
    """Every slot of a sliding plan from the definition (test_sliding_gpu._slots): [(chrom, j, begin, end)], slot j
    of a chromosome holding the SNPs with j s + 1 <= pos <= j s + w (pos 0: slot 0); begin == end: empty."""
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


def oracle_ref(p, wins, ocfg, bg_of, key=None):
    """(windows, O.window_records, O.window_fst per window); with ``key`` computed once and shared."""
    if key is not None and key in _REF:
        return _REF[key]
    recs = O.window_records(p, wins, ocfg, bg_of)
    fst = [O.window_fst(p, np.arange(w[-2], w[-1]), ocfg) for w in wins]
    ref = (wins, recs, fst)
    if key is not None:
        _REF[key] = ref
    return ref


def wide_scale(n):
    """The `wide` rule of test_null_gpu._check: with N in the 1e5 .. 1e6 range S and N ln N are sums of tens of
    rounded terms of that size, so either side carries ~100 eps N ln N of absolute error; the relative 1e-10 is
    taken of max(|T|, 1e-4 N ln N)."""
    return 1e-4 * n * math.log(n) if n > 1 else 0.0


def check_records(recs, fst, ref, wide=False, fst_tol=None):
    """Every non-empty record (the Q9 helper aside) against ref = (windows, oracle records, oracle Fst), in scan
    order: chrom / begin / end and the five integer fields exact, T2D / T1D by golden_util.close (``wide``: of
    max(|T|, 1e-4 N ln N), see wide_scale), 0 or NaN where the oracle has None; Fst (``fst`` None: not checked)
    within 1e-12 + 1e-10 |x| of the oracle's (``fst_tol(i)``: a larger absolute bound for window i, added to it),
    NaN exactly where the oracle has None and in every empty slot."""
    from sfs2d import _lib as L
    wins, orec, ofst = ref
    live = (recs["flags"] & (L.W_EMPTY | L.W_EXTRA)) == 0
    body = recs[live]
    assert len(body) == len(wins), (len(body), len(wins))
    fl = [None] * len(wins)
    if fst is not None:
        assert np.all(np.isnan(fst[: len(live)][~live[: len(fst)]]))
        fl = fst[: len(live)][live[: len(fst)]]
        assert len(fl) == len(wins)
    for i, (w, r, o, f) in enumerate(zip(wins, body, orec, ofst)):
        assert (int(r["chrom"]), int(r["begin"]), int(r["end"])) == (w[0], w[-2], w[-1]), (i, w)
        for a, b in (("snp_count", "snp_count"), ("n2", "N2"), ("n2_all", "N2_all"), ("n1a", "N1a"), ("n1b", "N1b")):
            assert int(r[a]) == o[b], (i, a, int(r[a]), o[b])
        for a, b, n in (("t2d", "T2D", "N2"), ("t1d_p1", "T1D_p1", "N1a"), ("t1d_p2", "T1D_p2", "N1b")):
            v = float(r[a])
            if o[b] is None:   # an empty spectrum: the record holds 0 or NaN (the host post-pass reports None)
                assert v == 0.0 or np.isnan(v), (i, a, v)
            else:
                assert gu.close(v, o[b], scale=wide_scale(o[n]) if wide else None), (i, a, v, o[b])
        if fst is None:
            continue
        g = float(fl[i])
        tol = 0.0 if fst_tol is None or f is None else fst_tol(i)
        assert (np.isnan(g) if f is None else abs(g - f) <= 1e-12 + 1e-10 * abs(f) + tol), (i, "fst", g, f, tol)


def check_against_oracle(recs, fst, p, wins, ocfg, bg_of, key=None, wide=False, fst_tol=None):
    """check_records against the oracle's records and Fst of ``wins`` ((chrom, ..., begin, end) tuples in scan
    order; bg_of(chrom) -> (2D, folded 1D, folded 1D) background)."""
    ref = oracle_ref(p, wins, ocfg, bg_of, key)
    check_records(recs, fst, ref, wide=wide, fst_tol=fst_tol)
    return ref


def same_ints(a, b):
    """Two record tables agree in every integer field and flag."""
    assert len(a) == len(b), (len(a), len(b))
    for k in INTS:
        bad = np.nonzero(a[k] != b[k])[0]
        assert bad.size == 0, (k, bad[:5], a[k][bad[:5]], b[k][bad[:5]])


def no_cancelled_t(recs):
    """No oracle T in (0, 1e-2): below that the absolute rounding error of any evaluation order (~1e-12 on sums
    of terms up to ~2e4) passes 1e-10 relative (test_filtered_plans._no_cancelled_t)."""
    for o in recs:
        for t in ("T2D", "T1D_p1", "T1D_p2"):
            v = o[t]
            assert v is None or v == 0.0 or not np.isfinite(v) or abs(v) >= 1e-2, (t, v)


def full_windows(recs):
    """Oracle records with all three statistics not None."""
    return sum(1 for o in recs if None not in (o["T2D"], o["T1D_p1"], o["T1D_p2"]))
