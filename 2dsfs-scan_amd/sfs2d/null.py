"""Bootstrap null of T2D / T1D: host side.

The null of a window of m SNPs from pool P (a chromosome, or -1 = the whole data set) is the
distribution of the same statistics over windows of m SNPs drawn with replacement from P's SNPs and
evaluated against the same background table.  The device draws and evaluates the replicates
(kernel k_null through ``Plan.null_run``); this module holds what surrounds it:

* ``size_classes`` -- the window sizes that get a null of their own (a window uses the smallest
  class >= its size);
* ``draw_indices`` -- the bit-exact host twin of the device's draws (``synth._philox``), single SNPs or
  blocks of consecutive SNPs (``block``: kernel k_null_blk, a null that keeps the pool's linkage);
* ``resample`` -- the replicate windows materialised as a ``PackedSNPs`` (for a CPU checker);
* ``pvalues`` -- the p-value definition in numpy; ``pvalues_device`` -- the same counts taken with
  torch sort / searchsorted over the record buffer in HBM.

Not in the reference, which thresholds windows outside its code (ECBstats_plots.R:45-50, 147-219).
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib as L
from .pack import PackedSNPs
from .synth import _M, _philox

STATS = ("T2D", "T1D_pop1", "T1D_pop2", "new_term_pop1", "new_term_pop2", "T2D_diff")
P_KEYS = tuple("p_" + s for s in STATS)
SLACK = 1e-9            # relative slack of the exceedance test (the fast and the exact path agree to 1e-10)
MAX_CALL_RECORDS = 1 << 22   # records one sfs2d_plan_null_run call writes (Plan.null_run splits above it)


# ----------------------------------------------------------------------------- size classes

def default_grid(max_m: int) -> np.ndarray:
    """g0 = 1, g(k+1) = max(g(k) + 1, ceil(g(k) * 2**(1/8))), up to the first term >= max_m: every m maps
    to a class at most 2**(1/8) - 1 = 9.05 % larger."""
    g = [1]
    while g[-1] < max_m:
        g.append(max(g[-1] + 1, math.ceil(g[-1] * 2.0 ** 0.125)))
    return np.array(g, np.int64)


def size_classes(ms, sizes=None) -> np.ndarray:
    """The class size of every window size in ``ms`` (int64, same shape): the smallest class >= m.
    ``sizes`` None: the default grid; "exact": every m is its own class; else a sorted list of class
    sizes that reaches max(ms) (ValueError otherwise).  Only the classes returned are ever run."""
    ms = np.asarray(ms, np.int64)
    if ms.size == 0:
        return ms.copy()
    if ms.min() < 1:
        raise ValueError("window sizes must be >= 1")
    if isinstance(sizes, str):
        if sizes != "exact":
            raise ValueError(f"sizes must be None, 'exact' or a sorted list, got {sizes!r}")
        return ms.copy()
    if sizes is None:
        grid = default_grid(int(ms.max()))
    else:
        grid = np.asarray(list(sizes), np.int64)
        if grid.size == 0 or np.any(np.diff(grid) <= 0) or grid[0] < 1:
            raise ValueError("sizes must be a strictly increasing list of sizes >= 1")
        if grid[-1] < ms.max():
            raise ValueError(f"sizes stop at {int(grid[-1])}, below the largest window ({int(ms.max())} SNPs)")
    return grid[np.searchsorted(grid, ms, side="left")]


# ----------------------------------------------------------------------------- draws (host twin)

def _mulhi64(x: np.ndarray, n: int) -> np.ndarray:
    """floor(x * n / 2**64) for uint64 x and 1 <= n < 2**32, in uint64 arithmetic."""
    n = np.uint64(n)
    hi, lo = x >> np.uint64(32), x & _M
    return (hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32)


def draw_indices(seed: int, pool_id: int, lo: int, n: int, m: int, replicates: int, block: int = 1) -> np.ndarray:
    """SNP indices of the ``replicates`` windows of task (pool_id, m): int64 [replicates, m].  Draw j of
    replicate r: c = philox4x32((j >> 1, r, m, pool_id + 1), (seed lo, seed hi)); x64 = c0 | c1 << 32 for
    even j, c2 | c3 << 32 for odd j; index = lo + mulhi64(x64, n).  A function of (seed, pool_id, m, r, j)
    alone -- what k_null computes.
    ``block`` = b > 1 (the block null, k_null_blk): that value is the start s_i of block i, for
    i < ceil(m / b) (b is not part of the counter), and draw j = i * b + k, k < b, is
    lo + (s_i + k) mod n -- runs of b consecutive SNPs of the circular pool, the last one cut at m."""
    if not (1 <= n < (1 << 32)) or m < 1 or replicates < 1:
        raise ValueError("draw_indices: 1 <= n < 2**32, m >= 1, replicates >= 1")
    if not (1 <= block < (1 << 32)):
        raise ValueError("draw_indices: 1 <= block < 2**32")
    b = int(block)
    nblk = -(-m // b)
    i = np.arange(nblk, dtype=np.uint64)[None, :]
    r = np.arange(replicates, dtype=np.uint64)[:, None]
    q = np.broadcast_to(i >> np.uint64(1), (replicates, nblk))
    rr = np.broadcast_to(r, (replicates, nblk))
    c0, c1, c2, c3 = _philox(q, rr, np.uint64(m & 0xFFFFFFFF), np.uint64((pool_id + 1) & 0xFFFFFFFF),
                             seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    even = (i & np.uint64(1)) == 0
    x = np.where(even, c0 | (c1 << np.uint64(32)), c2 | (c3 << np.uint64(32)))
    s = _mulhi64(x, n)
    if b > 1:
        j = np.arange(m, dtype=np.uint64)
        s = (s[:, j // np.uint64(b)] + (j % np.uint64(b))[None, :]) % np.uint64(n)   # (s + k < 2**33)
    return (np.uint64(lo) + s).astype(np.int64)


def pool_range(p: PackedSNPs, pool: int):
    """(lo, n) of pool ``pool`` of data set p: chromosome pool's SNP range, or everything for -1."""
    if pool == -1:
        return 0, p.n
    if not 0 <= pool < p.nchrom:
        raise ValueError(f"pool {pool} out of range")
    return int(p.chrom_off[pool]), int(p.chrom_off[pool + 1] - p.chrom_off[pool])


def resample(p: PackedSNPs, tasks, replicates: int, seed: int, block: int = 1):
    """The replicate windows of ``tasks`` ((pool, m) pairs) as a data set: (PackedSNPs q, wins) with
    wins[t * replicates + r] = (pool, r, begin, end), SNPs [begin, end) of q being replicate r of task t
    (each drawn SNP with its own counts, position and annotation; one pseudo-chromosome per task).  For a
    CPU checker of the device records (tests: oracle.window_records(q, wins, ...)); the device never
    materialises these windows.  ``block``: the block length of ``draw_indices``."""
    idx, wins, offs = [], [], [0]
    for pool, m in tasks:
        lo, n = pool_range(p, int(pool))
        if n == 0:
            raise ValueError(f"pool {pool} is empty")
        d = draw_indices(seed, int(pool), lo, n, int(m), replicates, block)
        for r in range(replicates):
            b = offs[-1] + r * int(m)
            wins.append((int(pool), r, b, b + int(m)))
        idx.append(d.reshape(-1))
        offs.append(offs[-1] + d.size)
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    q = PackedSNPs(p.counts[idx], p.pos[idx], np.array(offs, np.int64), [f"task{t:05d}" for t in range(len(offs) - 1)],
                   p.ann_id[idx], list(p.ann_names), p.pop1, p.pop2)
    return q, wins


# ----------------------------------------------------------------------------- p-values

def record_stats(recs: np.ndarray) -> np.ndarray:
    """The six statistics of every record, float64 [6, n] in STATS order, NaN where invalid ("None":
    N == 0 or a BG-zero flag; a derived term with any invalid operand).  A valid statistic that is itself
    NaN (scipy's negative p[-1]) becomes +inf-free NaN too: it exceeds nothing and nothing exceeds it."""
    fl = recs["flags"]
    t2 = np.where((recs["n2"] == 0) | ((fl & L.W_BG2_ZERO) != 0), np.nan, recs["t2d"])
    ta = np.where((recs["n1a"] == 0) | ((fl & L.W_BG1A_ZERO) != 0), np.nan, recs["t1d_p1"])
    tb = np.where((recs["n1b"] == 0) | ((fl & L.W_BG1B_ZERO) != 0), np.nan, recs["t1d_p2"])
    with np.errstate(invalid="ignore"):
        return np.stack([t2, ta, tb, t2 - ta, t2 - tb, t2 - (ta + tb) / 2])


def valid_mask(recs: np.ndarray) -> np.ndarray:
    """bool [6, n]: which statistics of a record are valid (not "None"), whatever their value."""
    fl = recs["flags"]
    v2 = (recs["n2"] != 0) & ((fl & L.W_BG2_ZERO) == 0)
    va = (recs["n1a"] != 0) & ((fl & L.W_BG1A_ZERO) == 0)
    vb = (recs["n1b"] != 0) & ((fl & L.W_BG1B_ZERO) == 0)
    return np.stack([v2, va, vb, v2 & va, v2 & vb, v2 & va & vb])


def _threshold(t):
    """t - SLACK * max(1, |t|); an infinite t is its own threshold."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(t), t - SLACK * np.maximum(1.0, np.abs(t)), t)


def _pools(obs_records, pools):
    if pools is None:
        pools = obs_records["chrom"].astype(np.int64)
    pools = np.asarray(pools, np.int64)
    return np.where(pools == 0xFFFFFFFF, -1, pools)


def pvalues(obs_records: np.ndarray, null_records: np.ndarray, classes, pools=None) -> dict:
    """{"p_T2D": float64 [n], ...} for the observed window records: p = (1 + #{r: t*_r valid and
    t*_r >= t - 1e-9 max(1, |t|)}) / (R + 1) over the R null records of the window's task
    (pool = its ``chrom``, or ``pools`` per record when one chromosome is every window's background;
    m = its class in ``classes``); NaN stands for None (invalid observed value).
    An invalid null value never counts and stays in the denominator.  The derived statistics are formed
    from each record's own three T's, invalid when any operand is.  Null records: ``chrom`` = pool
    (0xffffffff: -1), ``end`` = m, one per replicate."""
    classes = np.asarray(classes, np.int64)
    ot, ov = record_stats(obs_records), valid_mask(obs_records)
    nt, nv = record_stats(null_records), valid_mask(null_records)
    out = np.full((6, len(obs_records)), np.nan)
    okey = (_pools(obs_records, pools) + 1) << 32 | classes
    nkey = (_pools(null_records, None) + 1) << 32 | null_records["end"].astype(np.int64)
    for key in np.unique(okey):
        o = np.nonzero(okey == key)[0]
        z = np.nonzero(nkey == key)[0]
        if z.size == 0:
            raise ValueError(f"no null records for pool {(key >> 32) - 1}, m {key & 0xffffffff}")
        for s in range(6):
            thr = _threshold(ot[s, o])
            ok = nv[s, z]
            with np.errstate(invalid="ignore"):
                k = ((nt[s, z][None, :] >= thr[:, None]) & ok[None, :]).sum(axis=1)
            out[s, o] = np.where(ov[s, o], (1.0 + k) / (z.size + 1.0), np.nan)
    return {name: out[s] for s, name in enumerate(P_KEYS)}


def pvalues_device(obs_records: np.ndarray, classes, null_buf, tasks, replicates: int, pools=None) -> dict:
    """``pvalues`` with the null records left on the device: ``null_buf`` a torch uint8 tensor holding
    len(tasks) * replicates records (task-major, as Plan.null_run(out_dev_ptr=...) writes them), ``tasks``
    the (pool, m) pairs in buffer order.  Per task the null values are sorted once on the device and the
    observed windows' exceedance counts taken by searchsorted; only the counts come back."""
    import torch

    classes = np.asarray(classes, np.int64)
    R, T = int(replicates), len(tasks)
    dev = null_buf.device
    f = null_buf.view(torch.float64).view(T, R, 8)
    i = null_buf.view(torch.int32).view(T, R, 16)
    fl = i[..., 9]
    v2 = (i[..., 5] != 0) & ((fl & L.W_BG2_ZERO) == 0)
    va = (i[..., 7] != 0) & ((fl & L.W_BG1A_ZERO) == 0)
    vb = (i[..., 8] != 0) & ((fl & L.W_BG1B_ZERO) == 0)
    t2, ta, tb = f[..., 5], f[..., 6], f[..., 7]
    vals = torch.stack([t2, ta, tb, t2 - ta, t2 - tb, t2 - (ta + tb) / 2])           # [6, T, R]
    ok = torch.stack([v2, va, vb, v2 & va, v2 & vb, v2 & va & vb])
    # what can never count (invalid, or a NaN value) becomes +inf: it sorts to the end, at or above every
    # threshold, so of the R - pos values at or above a threshold nn - pos are countable ones
    can = ok & ~torch.isnan(vals)
    inf = torch.tensor(math.inf, dtype=torch.float64, device=dev)
    svals, _ = torch.sort(torch.where(can, vals, inf), dim=2)
    nn = can.sum(dim=2)                                                              # [6, T]
    ot, ov = record_stats(obs_records), valid_mask(obs_records)
    thr = _threshold(ot)
    tix = {(int(pool), int(m)): t for t, (pool, m) in enumerate(tasks)}
    pools = _pools(obs_records, pools)
    ti = np.array([tix[(int(a), int(b))] for a, b in zip(pools, classes)], np.int64)
    order = np.argsort(ti, kind="stable")
    thr_d = torch.from_numpy(np.ascontiguousarray(thr[:, order])).to(dev)
    k_d = torch.zeros(thr_d.shape, dtype=torch.int64, device=dev)
    bounds = np.searchsorted(ti[order], np.arange(T + 1))
    for t in range(T):
        a, b = int(bounds[t]), int(bounds[t + 1])
        if a == b:
            continue
        th = thr_d[:, a:b].contiguous()
        pos = torch.searchsorted(svals[:, t, :].contiguous(), th, side="left")
        cnt = nn[:, t, None] - torch.minimum(pos, nn[:, t, None])
        k_d[:, a:b] = torch.where(torch.isnan(th), torch.zeros_like(cnt), cnt)   # (a NaN observed value exceeds nothing)
    k = np.empty((6, len(obs_records)), np.int64)
    k[:, order] = k_d.cpu().numpy()
    out = np.where(ov, (1.0 + k) / (R + 1.0), np.nan)
    return {name: out[s] for s, name in enumerate(P_KEYS)}
