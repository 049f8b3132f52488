"""The null of the projected scan: p-values from replicates that keep each window's called counts (k_proj_null,
csrc/sfs2d_projnull.hpp; ``Plan.project_null``).

The projected T of a window (``Plan.project_scan``) still grows as the called counts of its SNPs approach the
projection (m1, m2): a SNP called in exactly m alleles adds an indicator to the projected grid, one called in n > m
a spread-out hypergeometric row.  Neither section 14's null design nor any other that redraws SNPs whatever their
coverage can judge it.  Here every used SNP of a window is replaced by one drawn among the used SNPs of its
chromosome with the SAME called-count pair (n1c, n2c); under missingness independent of frequency such SNPs are
exchangeable, so the null is exact conditional on the window's coverage.

  pool, stratum   the pool of chromosome c is its used SNPs (member & n1c >= m1 & n2c >= m2, section 19's); the
                  stratum of a used SNP is the set of the pool's SNPs with the same (n1c, n2c), in ascending SNP
                  index -- never empty, the SNP itself is in it
  entry           a record index s of the plan's last run; R replicates each, record t R + r
  slot i          of replicate r: SNP begin + i of the record's clamped range; an unused SNP draws nothing; a used
                  one with stratum (start, size) draws
                    c = philox4x32((i >> 1, r, s, chrom + 1), (seed & 0xffffffff, seed >> 32));
                    x64 = c0 | c1 << 32 (i even), c2 | c3 << 32 (i odd);
                    SNP pool_idx[start + mulhi64(x64, size)]
  record          what the projected scan gives for a window made of the drawn SNPs, against the record's chromosome;
                  n_used / n_dropped are the window's
  thin            per entry, the used slots whose stratum holds fewer than ``L.PNULL_THIN`` SNPs
  p-value         section 14's rule on the six statistics formed as ``spectra.project_scan_rows`` forms them:
                  p = (1 + #{r : t*_r not NaN and t*_r >= t - 1e-9 max(1, |t|)}) / (R + 1); an infinite t is its own
                  threshold; an observed NaN / None gives None

``strata`` / ``conditional_draws`` are the bit-exact host twins of the pool build and the draws, ``project_null_np``
the twin of the records, ``project_pvalues`` / ``project_pvalues_device`` the p-values, ``add_pvalue_columns`` the
result rows' seven extra columns.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from . import _lib as L
from . import spectra as SP
from .diversity import _filter_mask
from .null import _mulhi64, _threshold
from .pack import PackedSNPs
from .synth import _philox

__all__ = ["Strata", "strata", "conditional_draws", "project_null_np", "project_pvalues", "project_pvalues_device",
           "add_pvalue_columns", "PROJ_P_KEYS", "PROJNULL_COLUMNS"]

PROJ_STATS = ("T2D_proj", "T1D_pop1_proj", "T1D_pop2_proj", "new_term_pop1_proj", "new_term_pop2_proj", "T2D_diff_proj")
PROJ_P_KEYS = tuple("p_" + s for s in PROJ_STATS)
PROJNULL_COLUMNS = list(PROJ_P_KEYS) + ["n_thin"]

# pool_idx[c]: the used SNPs of chromosome c (data-set indices) sorted by (n1c, n2c), stable; start / size: per SNP
# of the data set, its stratum's first position in pool_idx[chrom] and length (-1 / 0: not used); used / member: bool
# per SNP; chrom: per SNP
Strata = namedtuple("Strata", "pool_idx start size used member chrom")


def _called(p):
    c = p.counts
    nc1 = ((c & np.uint32(0xFF)) + ((c >> np.uint32(8)) & np.uint32(0xFF))).astype(np.int64)
    nc2 = (((c >> np.uint32(16)) & np.uint32(0xFF)) + (c >> np.uint32(24))).astype(np.int64)
    return nc1, nc2


def _member_mask(p, cfg):
    """bool per SNP: the scan's own membership (spectra._members' rule), over the whole data set."""
    c = p.counts
    r1, a1, r2, a2 = [((c >> np.uint32(s)) & np.uint32(0xFF)).astype(np.int64) for s in (0, 8, 16, 24)]
    x1, x2 = a1, a2
    if cfg.fold:
        sw = (a1 + a2) > (int(cfg.n1p) + int(cfg.n2p))
        x1, x2 = np.where(sw, r1, a1), np.where(sw, r2, a2)
    return _filter_mask(p, 0, p.n, cfg) & ((x1 != 0) | (x2 != 0))


def strata(p, cfg, m1: int, m2: int) -> Strata:
    """The pools and strata of data set ``p`` under ``cfg`` at the projection (m1, m2): the host twin of the pool
    build (a stable sort of each chromosome's used SNPs by (n1c, n2c))."""
    m1, m2 = int(m1), int(m2)
    nc1, nc2 = _called(p)
    member = _member_mask(p, cfg)
    used = member & (nc1 >= m1) & (nc2 >= m2)
    start, size = np.full(p.n, -1, np.int64), np.zeros(p.n, np.int64)
    chrom = np.zeros(p.n, np.int64)
    pools = []
    for c in range(p.nchrom):
        lo, hi = int(p.chrom_off[c]), int(p.chrom_off[c + 1])
        chrom[lo:hi] = c
        idx = lo + np.nonzero(used[lo:hi])[0]
        key = nc1[idx] * 1024 + nc2[idx]
        order = np.argsort(key, kind="stable")
        pool, ks = idx[order], key[order]
        pools.append(pool.astype(np.int64))
        if len(pool):
            head = np.concatenate([[True], ks[1:] != ks[:-1]])
            first = np.nonzero(head)[0]
            seg = np.cumsum(head) - 1
            length = np.diff(np.concatenate([first, [len(pool)]]))
            start[pool], size[pool] = first[seg], length[seg]
    return Strata(pools, start, size, used, member, chrom)


def _rec_range(r, n):
    hi = min(int(r["end"]), n)
    return min(int(r["begin"]), hi), hi


def conditional_draws(p, recs, cfg, m1: int, m2: int, rec=None, replicates: int = 1, seed: int = 0, st: Strata = None):
    """The drawn SNPs of ``replicates`` replicates of the entries ``rec`` (None: every record): a list with one int64
    array [replicates, end - begin] per entry, -1 where the slot draws nothing (an unused SNP); an EMPTY / EXTRA
    record gives an array of no slots.  Bit-exact host twin of k_proj_null's draws (module docstring)."""
    R = int(replicates)
    if R < 1:
        raise ValueError("conditional_draws: replicates >= 1")
    st = strata(p, cfg, m1, m2) if st is None else st
    rec = np.arange(len(recs), dtype=np.int64) if rec is None else np.asarray(rec, np.int64).reshape(-1)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    out = []
    rr = np.arange(R, dtype=np.uint64)[:, None]
    for s in rec.tolist():
        if not 0 <= s < len(recs):
            raise ValueError(f"record {s} outside [0, {len(recs)})")
        r = recs[s]
        if int(r["flags"]) & (L.W_EMPTY | L.W_EXTRA):
            out.append(np.zeros((R, 0), np.int64))
            continue
        b, e = _rec_range(r, p.n)
        c = int(r["chrom"])
        i = np.arange(e - b, dtype=np.uint64)[None, :]
        q = np.broadcast_to(i >> np.uint64(1), (R, e - b))
        c0, c1, c2, c3 = _philox(q, np.broadcast_to(rr, (R, e - b)), np.uint64(s & 0xFFFFFFFF),
                                 np.uint64((c + 1) & 0xFFFFFFFF), k0, k1)
        x = np.where((i & np.uint64(1)) == 0, c0 | (c1 << np.uint64(32)), c2 | (c3 << np.uint64(32)))
        used = st.used[b:e]
        size = np.where(used, st.size[b:e], 1).astype(np.uint64)
        off = _mulhi64(x, size[None, :]).astype(np.int64)   # (a size per slot)
        d = np.full((R, e - b), -1, np.int64)
        if used.any():
            pool = st.pool_idx[c]
            at = st.start[b:e][None, :] + off
            d[:, used] = pool[at[:, used]]
        out.append(d)
    return out


def _weights_float(n, a, m):
    """h(j; n, a, m), j = 0 .. m, float64: each the exact ratio rounded once."""
    return np.array([float(w) for w in SP.project_weights_exact(n, a, m)], np.float64)


def _stats_float(grids, bg, fold):
    """(t2d, t1d_p1, t1d_p2, n2, n1a, n1b), float64 [R] each, of the unfolded grids [R, m1 + 1, m2 + 1] against the
    unfolded background grid ``bg``: section 19's closed form, vectorised (NaN: N = 0 or B = 0; +inf: a touched bin
    the background lacks)."""
    m1, m2 = bg.shape[0] - 1, bg.shape[1] - 1
    g = SP.fold_projected(grids) if fold else np.asarray(grids)
    b = SP.fold_projected(bg) if fold else np.asarray(bg)
    in1 = [j for j in range(1, m1 + 1) if 2 * j < m1]
    in2 = [j for j in range(1, m2 + 1) if 2 * j < m2]

    def spectra3(z):
        s1, s2 = SP.projected_marginals(z)
        return (z.reshape(z.shape[:-2] + (-1,))[..., 1:-1], SP.fold1d_projected(s1)[..., in1],
                SP.fold1d_projected(s2)[..., in2])
    out_t, out_n = [], []
    for x, y in zip(spectra3(g), spectra3(b)):
        N, B = x.sum(axis=-1), float(np.sum(y))
        with np.errstate(divide="ignore", invalid="ignore"):
            lx = np.log(x / N[:, None])
            ly = np.log(y / B) if B > 0 else np.full(y.shape, np.nan)
            term = np.where(x > 0, x * (lx - ly[None, :]), 0.0)
            t = 2.0 * term.sum(axis=-1)
        t = np.where(((x > 0) & (y == 0)[None, :]).any(axis=-1), np.inf, t)
        t = np.where((N == 0) | (B == 0), np.nan, t)
        out_t.append(t)
        out_n.append(N)
    return tuple(out_t) + tuple(out_n)


NULL_NP_DTYPE = np.dtype([("t2d", "<f8"), ("t1d_p1", "<f8"), ("t1d_p2", "<f8"), ("n2", "<f8"), ("n1a", "<f8"),
                          ("n1b", "<f8"), ("n_used", "<i8"), ("n_dropped", "<i8"), ("flags", "<u4")])


def project_null_np(p, recs, cfg, m1: int, m2: int, rec=None, replicates: int = 1, seed: int = 0, exact: bool = False,
                    draws=None, st: Strata = None):
    """The twin of ``Plan.project_null``: ``(records, thin)`` -- a structured array (``spectra.project_scan_np``'s
    fields), record t * replicates + r the replicate r of entry t, and the thin-slot count per entry.  The drawn SNPs
    (``conditional_draws``; ``draws``: given ones, one array per entry) are gathered into a data set of their own and
    projected as a window is.  ``exact``: through ``spectra.project_np`` with exact weights and rational sums, one
    logarithm per ratio (small cases); else float64 weights (each the exact ratio rounded once) and float64 sums,
    vectorised over the replicates."""
    m1, m2, R = int(m1), int(m2), int(replicates)
    st = strata(p, cfg, m1, m2) if st is None else st
    rec = np.arange(len(recs), dtype=np.int64) if rec is None else np.asarray(rec, np.int64).reshape(-1)
    if draws is None:
        draws = conditional_draws(p, recs, cfg, m1, m2, rec, R, seed, st)
    out = np.zeros(len(rec) * R, NULL_NP_DTYPE)
    thin = np.zeros(len(rec), np.uint32)
    fold = bool(cfg.fold)
    bgs = {}

    def background(c):
        if c not in bgs:
            g, _, _ = SP.project_np(p, recs, cfg, m1, m2, [-(c + 1)], [0], 1, exact=exact)
            bgs[c] = g[0]
        return bgs[c]
    W1 = W2 = None
    if not exact:   # per SNP of the data set its two weight vectors (used SNPs alone; equal counts share a row)
        c = p.counts
        r1, a1, r2, a2 = [((c >> np.uint32(s)) & np.uint32(0xFF)).astype(np.int64) for s in (0, 8, 16, 24)]
        W1, W2 = np.zeros((p.n, m1 + 1)), np.zeros((p.n, m2 + 1))
        for W, r_, a_, m in ((W1, r1, a1, m1), (W2, r2, a2, m2)):
            u = np.nonzero(st.used)[0]
            keys, inv = np.unique(np.stack([r_[u], a_[u]], axis=1), axis=0, return_inverse=True)
            tab = np.array([_weights_float(int(q + b), int(b), m) for q, b in keys.tolist()]).reshape(len(keys), m + 1)
            W[u] = tab[inv.reshape(-1)]
    in1 = [j for j in range(1, m1 + 1) if 2 * j < m1]
    in2 = [j for j in range(1, m2 + 1) if 2 * j < m2]
    for t, (s, d) in enumerate(zip(rec.tolist(), draws)):
        r = recs[s]
        fl = int(r["flags"]) & (L.W_EMPTY | L.W_EXTRA)
        if fl:
            out["flags"][t * R:(t + 1) * R] = fl
            continue
        b, e = _rec_range(r, p.n)
        c = int(r["chrom"])
        used = st.used[b:e]
        nu, nd = int(used.sum()), int((st.member[b:e] & ~used).sum())
        thin[t] = int((used & (st.size[b:e] < L.PNULL_THIN)).sum())
        d = np.asarray(d, np.int64).reshape(R, e - b)[:, used]   # [R, nu]
        o = out[t * R:(t + 1) * R]
        o["n_used"], o["n_dropped"] = nu, nd
        bg = background(c)
        if not exact:
            grids = np.matmul(W1[d].transpose(0, 2, 1), W2[d]) if nu else np.zeros((R, m1 + 1, m2 + 1))
            t2, ta, tb, n2, na, nb = _stats_float(grids, bg, fold)
            o["t2d"], o["t1d_p1"], o["t1d_p2"], o["n2"], o["n1a"], o["n1b"] = t2, ta, tb, n2, na, nb
            continue
        idx = d.reshape(-1)
        q = PackedSNPs(p.counts[idx], p.pos[idx], np.array([0, len(idx)], np.int64), ["draws"], p.ann_id[idx],
                       list(p.ann_names), p.pop1, p.pop2)
        qrecs = np.zeros(R, L.WINDOW_DTYPE)
        qrecs["begin"] = np.arange(R) * nu
        qrecs["end"] = qrecs["begin"] + nu
        grids, _, _ = SP.project_np(q, qrecs, cfg, m1, m2, exact=True)
        both = np.concatenate([grids, bg[None]])
        if fold:
            both = SP.fold_projected(both)
        s1, s2 = SP.projected_marginals(both)
        f1, f2 = SP.fold1d_projected(s1), SP.fold1d_projected(s2)
        flat = both.reshape(R + 1, -1)
        for k in range(R):
            t2, n2 = SP._llr(flat[k][1:-1].tolist(), flat[R][1:-1].tolist())
            ta, na = SP._llr([f1[k][j] for j in in1], [f1[R][j] for j in in1])
            tb, nb = SP._llr([f2[k][j] for j in in2], [f2[R][j] for j in in2])
            o[k] = (t2, ta, tb, float(n2), float(na), float(nb), nu, nd, 0)
    return out, thin


# ----------------------------------------------------------------------------- p-values

def _six(stats):
    """float64 [6, n]: the six statistics of projected-scan records as ``spectra.project_scan_rows`` forms them (NaN
    for None: a NaN statistic, a record that is no window, a derived term with a None operand or inf - inf)."""
    fl = (np.asarray(stats["flags"]) & (L.W_EMPTY | L.W_EXTRA)) != 0
    t2, ta, tb = (np.where(fl, np.nan, np.asarray(stats[k], np.float64)) for k in ("t2d", "t1d_p1", "t1d_p2"))
    with np.errstate(invalid="ignore"):
        return np.stack([t2, ta, tb, t2 - ta, t2 - tb, t2 - (ta + tb) / 2])


def project_pvalues(obs, null, replicates: int) -> dict:
    """{PROJ_P_KEYS: float64 [n]} of the observed projected-scan records ``obs`` (``Plan.project_scan``'s or the
    twin's) from their null records ``null`` (``Plan.project_null``'s or the twin's: ``replicates`` per observed
    record, record-major): p = (1 + #{r: t*_r not NaN and t*_r >= t - 1e-9 max(1, |t|)}) / (R + 1); an infinite t is
    its own threshold; NaN stands for None (an observed NaN / None)."""
    R = int(replicates)
    if R < 1 or len(null) != len(obs) * R:
        raise ValueError(f"project_pvalues: {len(null)} null records for {len(obs)} observed ones x {R} replicates")
    ot = _six(obs)                                   # [6, n]
    nt = _six(null).reshape(6, len(obs), R)          # [6, n, R]
    thr = _threshold(ot)
    with np.errstate(invalid="ignore"):
        k = ((nt >= thr[:, :, None]) & ~np.isnan(nt)).sum(axis=2)
    out = np.where(np.isnan(ot), np.nan, (1.0 + k) / (R + 1.0))
    return {name: out[s] for s, name in enumerate(PROJ_P_KEYS)}


def project_pvalues_device(obs, null_buf, replicates: int) -> dict:
    """``project_pvalues`` with the null records left on the device: ``null_buf`` a torch uint8 tensor holding
    len(obs) * replicates sfs2d_projstat records as ``Plan.project_null(out_dev_ptr=...)`` writes them.  The
    exceedance counts are taken on the device; only the counts come back."""
    import torch

    R, n = int(replicates), len(obs)
    if R < 1 or null_buf.numel() != n * R * L.PROJSTAT_DTYPE.itemsize:
        raise ValueError(f"project_pvalues_device: the buffer does not hold {n} x {R} records")
    f = null_buf.view(torch.float64).view(n, R, 8)
    fl = (null_buf.view(torch.int32).view(n, R, 16)[..., 14] & ((L.W_EMPTY | L.W_EXTRA) - (1 << 32))) != 0
    nan = torch.tensor(math.nan, dtype=torch.float64, device=null_buf.device)
    t2, ta, tb = (torch.where(fl, nan, f[..., k]) for k in (0, 1, 2))
    vals = torch.stack([t2, ta, tb, t2 - ta, t2 - tb, t2 - (ta + tb) / 2])   # [6, n, R]
    ot = _six(obs)
    thr = torch.from_numpy(np.ascontiguousarray(_threshold(ot))).to(null_buf.device)
    k = ((vals >= thr[:, :, None]) & ~torch.isnan(vals)).sum(dim=2).cpu().numpy()
    out = np.where(np.isnan(ot), np.nan, (1.0 + k) / (R + 1.0))
    return {name: out[s] for s, name in enumerate(PROJ_P_KEYS)}


def add_pvalue_columns(rows: dict, labels, pv: dict, thin) -> dict:
    """``rows`` (``spectra.project_scan_rows``'s, of the records that ``labels`` names, in their order) with the seven
    columns PROJNULL_COLUMNS added: ``pv`` / ``thin`` per record, at the labels' indices; a NaN p-value is None."""
    for i, lb in enumerate(labels):
        if lb is None:
            continue
        row = rows[lb]
        for k in PROJ_P_KEYS:
            v = float(pv[k][i])
            row[k] = None if math.isnan(v) else v
        row["n_thin"] = int(thin[i])
    return rows

