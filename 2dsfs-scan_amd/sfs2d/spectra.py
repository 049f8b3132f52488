"""Window spectra: the joint SFS of chosen windows, pooled or each, and what to do with them.

The GPU (k_spec_win, csrc/sfs2d_spec.hpp; ``Plan.spectra``) sums the 2D and folded 1D spectra of chosen records of
a plan's last run into groups (include/sfs2d.h, ``sfs2d_plan_spectra``).  This module holds
what is left for the host: taking a group's row apart (``split_row``), the numpy twin of the device sums
(``window_spectra_np``, the definition the tests compare against), choosing the outlier windows of a scan
(``select_top``), the per-bin comparison of a pooled foreground with its background (``residuals``) and dadi's
``.fs`` file format (``write_dadi_fs`` / ``read_dadi_fs``).

Per record with SNP range [begin, end), under the plan's position filter, variant_type filter and fold:

* 2D: the dense (2 n1p + 1) x (2 n2p + 1) grid of calculate_2d_sfs over the window, row-major (x1, x2); bin (0, 0)
  is 0 (those SNPs are skipped), the last bin (n1, n2) is counted;
* 1D, per population: the folded spectrum of raw alt counts at the inner bins 1 .. pop_size - 1 (the bins T1D
  reads); entries 0 and pop_size are 0.

A group is the SUM over its selection entries.  On overlapping windows (sliding windows, regions) that is a sum
over windows, not the spectrum of their union: a SNP inside two selected windows is counted twice.

Projected spectra (k_proj_win, csrc/sfs2d_proj.hpp; ``Plan.project``): the grid above bins a
SNP by its raw alt count whatever its called count, which a model fit (dadi, moments, fastsimcoal) cannot take
when calls are missing.  For a projection ``(m1, m2)`` of haploid sample sizes a member SNP (one the plan's run
counts in its 2D SFS) with called counts n_k = r_k + a_k >= m_k in both populations is *used* and adds
``h(j1; n1, a1, m1) h(j2; n2, a2, m2)``, ``h(j; n, a, m) = C(a, j) C(n - a, m - j) / C(n, m)``, to bin (j1, j2) of a
dense (m1 + 1) x (m2 + 1) grid; any other member is *dropped*.  The device returns the UNFOLDED grid of raw alt
counts; what is linear is done here: the joint fold (``fold_projected``: bin (j1, j2) with 2 (j1 + j2) > m1 + m2 is
added to (m1 - j1, m2 - j2); a tie stays where it is, as the scan's fold leaves it -- dadi's ``fold()`` AVERAGES
the two halves of a tie instead), the two 1D marginals (``projected_marginals``) and their folds
(``fold1d_projected``).  ``project_np`` is the exact twin (rational weights), the definition the tests compare
against.

The projected scan (k_proj_scan, csrc/sfs2d_projscan.hpp; ``Plan.project_scan``): T2D and T1D
of EVERY window at the common sample size, each window's projected grid (folded when the plan folds) against its
chromosome's.  With ``x = X.ravel()[1:-1]``, ``N = sum x``, ``B = sum b[1:-1]``: ``T2D = 2 sum_{x_k > 0} x_k (ln(x_k /
N) - ln(b_k / B))`` = ``pooled_t2d(residuals(X, b))``, +inf when a touched bin has b_k = 0, NaN exactly when N = 0 or
B = 0; T1D the same form on the folded marginal at its inner bins 1 <= j, 2 j < m_k.  The closed form is the
statistic: the reference's exact 0.0 for proportional spectra and scipy's NaN rule for an empty last bin are not
reproduced.  ``project_scan_np`` is the twin (tests only), ``project_scan_rows`` makes the result rows.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from . import _lib as L
from .diversity import _filter_mask

__all__ = ["split_row", "window_spectra_np", "select_top", "residuals", "pooled_t2d", "write_dadi_fs",
           "read_dadi_fs", "RESIDUAL_COLUMNS", "project_weights_exact", "project_np", "fold_projected",
           "projected_marginals", "fold1d_projected", "project_scan_np", "project_scan_rows", "PROJSCAN_COLUMNS"]

RESIDUAL_COLUMNS = ["x1", "x2", "fg_count", "bg_count", "fg_p", "bg_p", "diff", "t2d_term"]


def split_row(row, n1p: int, n2p: int):
    """(grid, folded1, folded2) of one group row [2D bins | pop-1 folded, n1p + 1 | pop-2 folded, n2p + 1]:
    the (2 n1p + 1, 2 n2p + 1) grid and the two folded 1D spectra (views of ``row``)."""
    row = np.asarray(row)
    g1, g2 = 2 * n1p + 1, 2 * n2p + 1
    nb2 = g1 * g2
    if row.ndim != 1 or row.size != L.spec_row_words(n1p, n2p):
        raise ValueError(f"a spectra row of pop sizes ({n1p}, {n2p}) has {L.spec_row_words(n1p, n2p)} words")
    return row[:nb2].reshape(g1, g2), row[nb2:nb2 + n1p + 1], row[nb2 + n1p + 1:]


def _record_row(p, lo, hi, cfg, n1p, n2p, fold):
    n1, n2 = 2 * n1p, 2 * n2p
    row = np.zeros(L.spec_row_words(n1p, n2p), np.int64)
    if hi <= lo:
        return row
    m = _filter_mask(p, lo, hi, cfg)
    c = p.counts[lo:hi][m]
    r1, a1, r2, a2 = [((c >> np.uint32(s)) & np.uint32(0xFF)).astype(np.int64) for s in (0, 8, 16, 24)]
    x1, x2 = a1, a2
    if fold:   # the joint fold on the SNP's own counts; a tie is not folded
        sw = (a1 + a2) > (n1p + n2p)
        x1, x2 = np.where(sw, r1, a1), np.where(sw, r2, a2)
    keep = (x1 != 0) | (x2 != 0)
    x1, x2 = x1[keep], x2[keep]
    if x1.size and (x1.max() > n1 or x2.max() > n2):
        raise ValueError("2D SFS bin outside the grid (allele counts exceed the declared sample size)")
    nb2 = (n1 + 1) * (n2 + 1)
    row[:nb2] = np.bincount(x1 * (n2 + 1) + x2, minlength=nb2)
    off = nb2
    for a, npop in ((a1, n1p), (a2, n2p)):
        a = a[a != 0]
        if a.size and a.max() > 2 * npop:
            raise KeyError(int(a.max()))
        f = np.minimum(a, 2 * npop - a)
        f = f[(f >= 1) & (f <= npop - 1)]
        row[off:off + npop + 1] = np.bincount(f, minlength=npop + 1)
        off += npop + 1
    return row


def window_spectra_np(p, recs, cfg, rec=None, grp=None, ngroups=None) -> np.ndarray:
    """The numpy twin of ``Plan.spectra``: ``int64[ngroups, row words]`` from the packed SNPs ``p``, the plan's
    window records ``recs`` and its configuration ``cfg`` (a ScanConfig, or an object with pop sizes ``n1p`` /
    ``n2p``, ``fold``, the position filter and ``variant_type``), with ``rec`` / ``grp`` / ``ngroups`` as
    ``Plan.spectra`` takes them."""
    n1p, n2p, fold = int(cfg.n1p), int(cfg.n2p), bool(cfg.fold)
    nrec = len(recs)
    rec = np.arange(nrec, dtype=np.int64) if rec is None else np.asarray(rec, np.int64).reshape(-1)
    grp = np.arange(len(rec), dtype=np.int64) if grp is None else np.asarray(grp, np.int64).reshape(-1)
    if len(rec) != len(grp):
        raise ValueError("rec and grp differ in length")
    if ngroups is None:
        ngroups = max(1, int(grp.max()) + 1 if len(grp) else 1)
    out = np.zeros((int(ngroups), L.spec_row_words(n1p, n2p)), np.int64)
    cache = {}
    for s, g in zip(rec.tolist(), grp.tolist()):
        if not 0 <= s < nrec or not 0 <= g < ngroups:
            raise ValueError(f"entry (record {s}, group {g}) out of range")
        r = recs[s]
        if int(r["flags"]) & (L.W_EMPTY | L.W_EXTRA):
            continue
        if s not in cache:
            hi = min(int(r["end"]), p.n)
            cache[s] = _record_row(p, min(int(r["begin"]), hi), hi, cfg, n1p, n2p, fold)
        out[g] += cache[s]
    return out


def project_weights_exact(n: int, a: int, m: int):
    """The hypergeometric weights h(j; n, a, m) = C(a, j) C(n - a, m - j) / C(n, m), j = 0 .. m, as exact
    Fractions (0 outside the support max(0, m - (n - a)) <= j <= min(m, a))."""
    n, a, m = int(n), int(a), int(m)
    if not (0 <= a <= n and 0 <= m <= n):
        raise ValueError(f"project_weights_exact: need 0 <= a <= n and 0 <= m <= n, got n={n} a={a} m={m}")
    den = math.comb(n, m)
    return [Fraction(math.comb(a, j) * math.comb(n - a, m - j), den) for j in range(m + 1)]


def _members(p, lo, hi, cfg, n1p, n2p, fold):
    """(r1, a1, r2, a2) int64 of the SNPs of [lo, hi) that the plan's run counts in its 2D SFS."""
    m = _filter_mask(p, lo, hi, cfg)
    c = p.counts[lo:hi][m]
    r1, a1, r2, a2 = [((c >> np.uint32(s)) & np.uint32(0xFF)).astype(np.int64) for s in (0, 8, 16, 24)]
    x1, x2 = a1, a2
    if fold:
        sw = (a1 + a2) > (n1p + n2p)
        x1, x2 = np.where(sw, r1, a1), np.where(sw, r2, a2)
    keep = (x1 != 0) | (x2 != 0)
    return r1[keep], a1[keep], r2[keep], a2[keep]


def _project_range(p, lo, hi, cfg, n1p, n2p, fold, m1, m2, D1, D2):
    """(grid of integers as an object array: the exact grid times D1 D2, n_used, n_dropped) of the SNP range
    [lo, hi).  D_k: a common multiple of C(n, m_k) over the called counts n >= m_k of the data set, so that every
    weight is an integer over D_k."""
    grid = np.zeros((m1 + 1, m2 + 1), object)
    if hi <= lo:
        return grid, 0, 0
    r1, a1, r2, a2 = _members(p, lo, hi, cfg, n1p, n2p, fold)
    used = (r1 + a1 >= m1) & (r2 + a2 >= m2)

    def weights(r, a, m, D):   # D h(j; r + a, a, m) over the support, as integers
        lo_j, hi_j = max(0, m - r), min(m, a)
        s = D // math.comb(r + a, m)
        return lo_j, np.array([math.comb(a, j) * math.comb(r, m - j) * s for j in range(lo_j, hi_j + 1)], object)
    # SNPs with equal counts add equal terms, and the sum factorises: per distinct (r1, a1) the outer product of
    # its pop-1 weights with the sum of the pop-2 weight vectors of its SNPs (each distinct (r2, a2) times its count)
    keys, cnt = np.unique(np.stack([r1[used], a1[used], r2[used], a2[used]], axis=1), axis=0, return_counts=True)
    by1, w2 = {}, {}
    for (q1, b1, q2, b2), k in zip(keys.tolist(), cnt.tolist()):
        if (q2, b2) not in w2:
            w2[(q2, b2)] = weights(q2, b2, m2, D2)
        l2, v2 = w2[(q2, b2)]
        v = by1.setdefault((q1, b1), np.zeros(m2 + 1, object))
        v[l2:l2 + len(v2)] += k * v2
    for (q1, b1), v in by1.items():
        l1, v1 = weights(q1, b1, m1, D1)
        nz = np.nonzero(v)[0]
        grid[l1:l1 + len(v1), nz[0]:nz[-1] + 1] += np.multiply.outer(v1, v[nz[0]:nz[-1] + 1])
    return grid, int(used.sum()), int((~used).sum())


def project_np(p, recs, cfg, m1: int, m2: int, rec=None, grp=None, ngroups=None, exact: bool = False):
    """The twin of ``Plan.project``, with exact weights: ``(float64[ngroups, m1 + 1, m2 + 1], used, dropped)`` from
    the packed SNPs ``p``, the plan's window records ``recs`` and its configuration ``cfg`` (as
    ``window_spectra_np`` takes them; ``cfg.fold`` decides membership alone -- the grid is unfolded).  Every weight
    is a ratio of ``math.comb`` values; the bins are summed as integers over one common denominator and divided
    once, correctly rounded.  ``rec[i] = -(c + 1)`` names the whole chromosome c.  ``exact``: return the grids as
    object arrays of Fractions."""
    n1p, n2p, fold = int(cfg.n1p), int(cfg.n2p), bool(cfg.fold)
    m1, m2 = int(m1), int(m2)
    if not (2 <= m1 <= 2 * n1p and 2 <= m2 <= 2 * n2p):
        raise ValueError(f"project: (m1, m2) = ({m1}, {m2}) outside [2, {2 * n1p}] x [2, {2 * n2p}]")
    nrec = len(recs)
    rec = np.arange(nrec, dtype=np.int64) if rec is None else np.asarray(rec, np.int64).reshape(-1)
    grp = np.arange(len(rec), dtype=np.int64) if grp is None else np.asarray(grp, np.int64).reshape(-1)
    if len(rec) != len(grp):
        raise ValueError("rec and grp differ in length")
    if ngroups is None:
        ngroups = max(1, int(grp.max()) + 1 if len(grp) else 1)
    ngroups = int(ngroups)
    c = p.counts
    nc1 = ((c & np.uint32(0xFF)) + ((c >> np.uint32(8)) & np.uint32(0xFF))).astype(np.int64)
    nc2 = (((c >> np.uint32(16)) & np.uint32(0xFF)) + (c >> np.uint32(24))).astype(np.int64)
    D1 = math.lcm(*[math.comb(n, m1) for n in np.unique(nc1[nc1 >= m1]).tolist()])
    D2 = math.lcm(*[math.comb(n, m2) for n in np.unique(nc2[nc2 >= m2]).tolist()])
    grids = np.zeros((ngroups, m1 + 1, m2 + 1), object)
    used, dropped = np.zeros(ngroups, np.int64), np.zeros(ngroups, np.int64)
    cache = {}
    for s, g in zip(rec.tolist(), grp.tolist()):
        if not -p.nchrom <= s < nrec or not 0 <= g < ngroups:
            raise ValueError(f"entry (record {s}, group {g}) out of range")
        if s < 0:
            lo, hi = int(p.chrom_off[-s - 1]), int(p.chrom_off[-s])
        else:
            r = recs[s]
            if int(r["flags"]) & (L.W_EMPTY | L.W_EXTRA):
                continue
            hi = min(int(r["end"]), p.n)
            lo = min(int(r["begin"]), hi)
        if (lo, hi) not in cache:
            cache[(lo, hi)] = _project_range(p, lo, hi, cfg, n1p, n2p, fold, m1, m2, D1, D2)
        gr, u, d = cache[(lo, hi)]
        grids[g] += gr
        used[g] += u
        dropped[g] += d
    D = D1 * D2
    flat = grids.ravel().tolist()
    if exact:
        out = np.empty(len(flat), object)
        out[:] = [Fraction(x, D) for x in flat]
        return out.reshape(grids.shape), used, dropped
    # (int / int: one correctly rounded division per bin)
    return np.array([x / D for x in flat], np.float64).reshape(grids.shape), used, dropped


def fold_projected(grid):
    """The joint fold of an unfolded projected grid (..., m1 + 1, m2 + 1): bin (j1, j2) with 2 (j1 + j2) > m1 + m2
    is added to (m1 - j1, m2 - j2) and zeroed; a tie, 2 (j1 + j2) == m1 + m2, stays where it is, as the scan's fold
    leaves a tied SNP (dadi's ``Spectrum.fold`` averages the two halves of a tie instead).  Linear: integer grids
    stay integer, object (Fraction) grids exact."""
    g = np.array(grid, copy=True)
    m1, m2 = g.shape[-2] - 1, g.shape[-1] - 1
    i, j = np.indices((m1 + 1, m2 + 1))
    hi = 2 * (i + j) > m1 + m2
    zero = 0 if g.dtype == object else g.dtype.type(0)
    return np.where(hi, zero, g) + np.where(hi, g, zero)[..., ::-1, ::-1]


def projected_marginals(grid):
    """The two 1D marginals (..., m1 + 1) and (..., m2 + 1) of an unfolded projected grid: the 1D projections of
    the used SNPs' raw alt counts to m1 and to m2 (a SNP's weights over the other population sum to 1)."""
    g = np.asarray(grid)
    return g.sum(axis=-1), g.sum(axis=-2)


def fold1d_projected(sfs1d):
    """The fold ``min(j, m - j)`` of an unfolded 1D projected spectrum (..., m + 1): entry j of the result, j <=
    m // 2, is ``x[j] + x[m - j]`` (``x[j]`` alone where j == m - j), the entries above m // 2 are 0."""
    x = np.asarray(sfs1d)
    m = x.shape[-1] - 1
    out = np.zeros_like(x)
    for j in range(m // 2 + 1):
        out[..., j] = x[..., j] if j == m - j else x[..., j] + x[..., m - j]
    return out


def _llr(x, b):
    """2 sum_{x_k > 0} x_k (ln(x_k / N) - ln(b_k / B)) of two equally long sequences of floats or Fractions, and N:
    NaN when N = 0 or B = 0, +inf when a bin with x_k > 0 has b_k = 0."""
    exact = len(x) > 0 and isinstance(x[0], Fraction)
    N, B = (sum(x), sum(b)) if exact else (math.fsum(x), math.fsum(b))
    if N == 0 or B == 0:
        return math.nan, N
    terms = []
    for xk, bk in zip(x, b):
        if xk > 0:
            if bk == 0:
                return math.inf, N
            terms.append(float(xk) * (math.log(xk / N) - math.log(bk / B)))
    return 2.0 * math.fsum(terms), N


def project_scan_np(p, recs, cfg, m1: int, m2: int, bg_chrom=None, exact: bool = False):
    """The twin of ``Plan.project_scan`` (tests only): a structured array, one entry per record, of ``t2d``,
    ``t1d_p1``, ``t1d_p2`` (float64), ``n2``, ``n1a``, ``n1b`` (the three N, float64), ``n_used``, ``n_dropped``
    and ``flags``, from ``project_np``'s grids of the records and of the chromosomes (``bg_chrom`` None: each record
    against its own chromosome; else chromosome index ``bg_chrom`` for every record), ``fold_projected`` when
    ``cfg.fold``, ``projected_marginals`` and ``fold1d_projected``.  ``exact``: the sums and ratios in rationals,
    one logarithm per ratio; else in float64 from the correctly rounded grids."""
    m1, m2 = int(m1), int(m2)
    nrec = len(recs)
    if bg_chrom is not None and not 0 <= int(bg_chrom) < p.nchrom:
        raise ValueError(f"project_scan: bg_chrom {bg_chrom} outside [0, {p.nchrom})")
    chroms = list(range(p.nchrom)) if bg_chrom is None else [int(bg_chrom)]
    rec = list(range(nrec)) + [-(c + 1) for c in chroms]
    grids, used, dropped = project_np(p, recs, cfg, m1, m2, rec, np.arange(len(rec)), len(rec), exact=exact)
    if cfg.fold:
        grids = fold_projected(grids)
    s1, s2 = projected_marginals(grids)
    f1, f2 = fold1d_projected(s1), fold1d_projected(s2)
    in1 = [j for j in range(1, m1 + 1) if 2 * j < m1]
    in2 = [j for j in range(1, m2 + 1) if 2 * j < m2]
    flat = grids.reshape(len(rec), -1)
    out = np.zeros(nrec, np.dtype([("t2d", "<f8"), ("t1d_p1", "<f8"), ("t1d_p2", "<f8"), ("n2", "<f8"), ("n1a", "<f8"),
                                   ("n1b", "<f8"), ("n_used", "<i8"), ("n_dropped", "<i8"), ("flags", "<u4")]))
    for i in range(nrec):
        fl = int(recs[i]["flags"]) & (L.W_EMPTY | L.W_EXTRA)
        if fl:
            out[i]["flags"] = fl
            continue
        g = nrec + (0 if bg_chrom is not None else int(recs[i]["chrom"]))
        t2, n2 = _llr(flat[i][1:-1].tolist(), flat[g][1:-1].tolist())
        ta, na = _llr([f1[i][j] for j in in1], [f1[g][j] for j in in1])
        tb, nb = _llr([f2[i][j] for j in in2], [f2[g][j] for j in in2])
        out[i] = (t2, ta, tb, float(n2), float(na), float(nb), int(used[i]), int(dropped[i]), 0)
    return out


PROJSCAN_COLUMNS = ["snp_count", "n_used", "n_dropped", "T2D_proj", "T1D_pop1_proj", "T1D_pop2_proj",
                    "new_term_pop1_proj", "new_term_pop2_proj", "T2D_diff_proj"]


def project_scan_rows(recs, stats, labels) -> dict:
    """{label: PROJSCAN_COLUMNS} of the labelled records of a projected scan: ``recs`` the plan's window records,
    ``stats`` ``Plan.project_scan``'s (or the twin's) at the same indices, ``labels`` one per record (None: a
    record that is no window of its own, left out).  A NaN statistic (an empty foreground or background) is None,
    +inf stays, a labelled record that is no window (an empty region) has None throughout; the differences follow the scans' clean None rules -- None when a statistic they read is None, and
    also where both are +inf (the difference is undefined)."""
    def val(v):
        v = float(v)
        return None if math.isnan(v) else v

    def diff(a, *b):
        if a is None or any(x is None for x in b):
            return None
        d = a - math.fsum(b) / len(b)
        return None if math.isnan(d) else d
    rows = {}
    for r, s, lb in zip(recs, stats, labels):
        if lb is None:
            continue
        if int(s["flags"]) & (L.W_EMPTY | L.W_EXTRA):   # (a region without SNPs: a row of its own, nothing to report)
            T2D = T1 = T2 = None
        else:
            T2D, T1, T2 = val(s["t2d"]), val(s["t1d_p1"]), val(s["t1d_p2"])
        rows[lb] = {"snp_count": int(r["snp_count"]), "n_used": int(s["n_used"]), "n_dropped": int(s["n_dropped"]),
                    "T2D_proj": T2D, "T1D_pop1_proj": T1, "T1D_pop2_proj": T2,
                    "new_term_pop1_proj": diff(T2D, T1), "new_term_pop2_proj": diff(T2D, T2),
                    "T2D_diff_proj": diff(T2D, T1, T2)}
    return rows


def select_top(rows: dict, key: str, q: float):
    """The labels of the rows of a scan's result dict whose ``key`` lies in the top 1 - q of its values, in scan
    order: candidates are the rows whose value is neither None nor NaN (+inf is kept: such a window is the most
    extreme there is), the threshold is ``numpy.quantile(values, q, method="higher")`` -- a value of the sample
    -- and a row is selected when its value >= the threshold (ties at the threshold are all in).  ValueError: q
    outside (0, 1), or no candidate."""
    q = float(q)
    if not 0.0 < q < 1.0:
        raise ValueError(f"select_top: q must lie in (0, 1), got {q}")
    cand = []
    for lb, row in rows.items():
        v = row.get(key)
        if v is None:
            continue
        v = float(v)
        if math.isnan(v):
            continue
        cand.append((lb, v))
    if not cand:
        raise ValueError(f"select_top: no row has a value of {key!r}")
    thr = float(np.quantile(np.array([v for _, v in cand], np.float64), q, method="higher"))
    return [lb for lb, v in cand if v >= thr]


def residuals(fg_grid, bg_grid) -> dict:
    """Per bin of the grid, a pooled foreground against its background: the two proportions over the inner bins
    (``ravel()[1:-1]``, the sum normalize_2d_sfs divides by), their difference, and the bin's term of T2D,
    ``2 x (ln(x / N) - ln(b / B))`` -- 0 where x = 0, +inf where x > 0 and b = 0; the terms sum to the pooled T2D
    (the multinomial coefficients of the two likelihoods cancel).  Returns a dict of arrays shaped like the grid:
    ``fg_count``, ``bg_count``, ``fg_p``, ``bg_p``, ``diff``, ``t2d_term``; the first and the last bin, which the
    statistic does not read, have proportions of their own counts over the same sums and a term of 0.  With an
    empty foreground or background (N = 0 or B = 0) the proportions over it and the terms are NaN."""
    fg = np.asarray(fg_grid)
    bg = np.asarray(bg_grid)
    if fg.shape != bg.shape or fg.ndim != 2:
        raise ValueError("residuals: two grids of one shape")
    x = fg.astype(np.float64).ravel()
    b = bg.astype(np.float64).ravel()
    N, B = math.fsum(x[1:-1].tolist()), math.fsum(b[1:-1].tolist())
    nan = np.full(x.shape, np.nan)
    fp = x / N if N > 0 else nan.copy()
    bp = b / B if B > 0 else nan.copy()
    term = nan.copy()
    if N > 0 and B > 0:
        term = np.zeros_like(x)
        inner = np.zeros(x.shape, bool)
        inner[1:-1] = True
        pos = inner & (x > 0)
        hit = pos & (b > 0)
        term[hit] = 2.0 * x[hit] * (np.log(fp[hit]) - np.log(bp[hit]))
        term[pos & ~(b > 0)] = np.inf
    sh = fg.shape
    return {"fg_count": fg.copy(), "bg_count": bg.copy(), "fg_p": fp.reshape(sh), "bg_p": bp.reshape(sh),
            "diff": (fp - bp).reshape(sh), "t2d_term": term.reshape(sh)}


def pooled_t2d(res: dict):
    """T2D of the pooled foreground against the background: the sum of ``residuals``' terms (None when either is
    empty)."""
    t = res["t2d_term"].ravel()
    if np.isnan(t).any():
        return None
    return math.inf if np.isinf(t).any() else math.fsum(t.tolist())


def residual_rows(res: dict):
    """The rows of the residual table, RESIDUAL_COLUMNS each: the bins where either count is non-zero, row-major."""
    fg, bg = res["fg_count"], res["bg_count"]
    out = []
    for i, j in zip(*np.nonzero((fg != 0) | (bg != 0))):
        f = fg[i, j].item()   # (an integer grid's count as int, as before; a projected grid's as the float it is)
        out.append([int(i), int(j), f if isinstance(f, float) else int(f), bg[i, j].item(), float(res["fg_p"][i, j]), float(res["bg_p"][i, j]),
                    float(res["diff"][i, j]), float(res["t2d_term"][i, j])])
    return out


def _fs_mask(d1: int, d2: int, folded: bool) -> np.ndarray:
    m = np.zeros((d1, d2), np.int64)
    m[0, 0] = m[d1 - 1, d2 - 1] = 1
    if folded:   # (n1 + n2) / 2 = n1p + n2p: the bins a folded spectrum cannot hold
        i, j = np.indices((d1, d2))
        m[i + j > (d1 - 1 + d2 - 1) // 2] = 1
    return m


def _fs_num(v) -> str:
    v = v.item() if hasattr(v, "item") else v
    return str(int(v)) if isinstance(v, (int, np.integer)) or float(v).is_integer() else repr(float(v))


def write_dadi_fs(path, grid, folded: bool, pop_ids=("pop1", "pop2")):
    """Write the 2D spectrum ``grid`` as a dadi ``.fs`` file (dadi.Spectrum.from_file reads it; moments too): three
    lines -- ``D1 D2 folded|unfolded "pop1" "pop2"``, the values row-major, the mask (1 = masked) at (0, 0), at
    (n1, n2) and, when ``folded``, where i + j > n1p + n2p."""
    g = np.asarray(grid)
    if g.ndim != 2:
        raise ValueError("write_dadi_fs: a 2D grid")
    if len(pop_ids) != 2 or any('"' in str(s) or "\n" in str(s) for s in pop_ids):
        raise ValueError("write_dadi_fs: two population ids without quotes or line breaks")
    d1, d2 = g.shape
    with open(path, "w") as f:
        f.write(f'{d1} {d2} {"folded" if folded else "unfolded"} "{pop_ids[0]}" "{pop_ids[1]}"\n')
        f.write(" ".join(_fs_num(v) for v in g.ravel()) + "\n")
        f.write(" ".join(str(int(v)) for v in _fs_mask(d1, d2, bool(folded)).ravel()) + "\n")


def read_dadi_fs(path):
    """Read a 2D ``.fs`` file: (grid, folded, pop_ids, mask).  ``grid`` is int64 when every value is an integer,
    else float64; comment lines (#) ahead of the header are skipped; ``mask`` is None when the file has no mask
    line."""
    with open(path) as f:
        lines = [ln.strip() for ln in f]
    lines = [ln for ln in lines if ln and not ln.startswith("#")]
    if len(lines) < 2:
        raise ValueError(f"{path}: not a dadi .fs file (header and values expected)")
    head, _, rest = lines[0].partition('"')
    tok = head.split()
    if len(tok) < 2:
        raise ValueError(f"{path}: header without two dimensions")
    dims, flags = [], []
    for t in tok:
        (dims if t.isdigit() else flags).append(t)
    if len(dims) != 2:
        raise ValueError(f"{path}: {len(dims)} dimensions (a 2D spectrum expected)")
    d1, d2 = int(dims[0]), int(dims[1])
    folded = "folded" in flags
    ids = ('"' + rest).split('"')[1::2] if rest else []
    vals = lines[1].split()
    if len(vals) != d1 * d2:
        raise ValueError(f"{path}: {len(vals)} values for a {d1} x {d2} grid")
    fv = np.array([float(v) for v in vals], np.float64)
    grid = fv.astype(np.int64) if np.all(np.isfinite(fv)) and np.all(fv == np.floor(fv)) else fv
    mask = None
    if len(lines) > 2:
        mv = lines[2].split()
        if len(mv) != d1 * d2:
            raise ValueError(f"{path}: {len(mv)} mask entries for a {d1} x {d2} grid")
        mask = np.array([int(v) for v in mv], np.int64).reshape(d1, d2)
    return grid.reshape(d1, d2), folded, tuple(ids), mask
