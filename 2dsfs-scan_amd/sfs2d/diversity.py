"""Per-window diversity: pi, dxy, Watterson's theta and Tajima's D beside the scan's statistics.

The GPU (k_div_win, csrc/sfs2d_div.hpp) sums per window, over the SNPs of the window's 2D SFS, functions of each
SNP's four allele counts (include/sfs2d.h, ``sfs2d_diversity``).  This module holds what is
left for the host: the numpy twin of those sums (``window_sums``, the definition the tests compare against),
Tajima's D from the fully called SNPs (``tajima_d``) and the per-site columns keyed by the scans' window labels
(``rows``).

Per SNP, population k with counts (r, a), n = r + a called alleles:

* pi_k term ``2 a r / (n (n - 1))`` for n >= 2, else 0 (the integer ``a r`` first: a fixed site adds exactly 0.0);
* S_k = 1 when n >= 2 and 0 < a < n;  theta_W,k term ``S_k / h(n)``, h(n) = sum_{i=1}^{n-1} 1 / i;
* dxy term ``(a1 r2 + r1 a2) / (n1 n2)`` for n1, n2 >= 1, else 0;
* fully called in k: n == 2 pop_size_k exactly -> ``S_full,k`` and ``AR_full,k = sum a r``.

The SNPs that take part pass the position and variant_type filters.  A SNP the 2D SFS drops as bin (0, 0) is fixed
for one allele in both populations after the fold, so all its terms are 0: the device may skip it, this twin does
not.

Per-site values divide the window's sums by its length in bp: the window size W for fixed-bp and sliding windows
(every one of the W sites is taken as callable: a SNP-only VCF knows nothing else), ``pos[end-1] - pos[begin] + 1``
for SNP-count windows, the region's own length ``last - first + 1`` for region windows.  S and Tajima's D are not
scaled.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib as L
from . import post

__all__ = ["KEYS", "harmonic", "tajima_d", "window_sums", "rows", "add_columns"]

# the columns every row gains (in CSV order)
KEYS = ["pi_pop1", "pi_pop2", "dxy", "da", "theta_w_pop1", "theta_w_pop2", "S_pop1", "S_pop2",
        "S_full_pop1", "S_full_pop2", "tajima_d_pop1", "tajima_d_pop2"]

_HMAX = 512   # called allele counts are u8 pairs: n <= 510


def harmonic(nmax: int = _HMAX) -> np.ndarray:
    """h[n] = sum_{i=1}^{n-1} 1 / i for n < nmax (h[0] = h[1] = 0), summed in ascending order of i -- the doubles
    the library's 1 / h(n) table is made from."""
    h = np.zeros(nmax, np.float64)
    acc = 0.0
    for n in range(2, nmax):
        acc += 1.0 / (n - 1)
        h[n] = acc
    return h


_H = harmonic()


def tajima_d(n, S, ar_sum):
    """Tajima's D (Tajima 1989) of ``S`` segregating sites in a sample of ``n`` sequences whose pairwise
    diversity is pi = 2 * ar_sum / (n (n - 1)), ``ar_sum`` = sum over the sites of alt count x ref count.
    None when S == 0 or the variance term is not positive (n < 4)."""
    n, S = int(n), int(S)
    if S <= 0 or n < 4:
        return None
    a1 = sum(1.0 / i for i in range(1, n))
    a2 = sum(1.0 / (i * i) for i in range(1, n))
    b1 = (n + 1) / (3.0 * (n - 1))
    b2 = 2.0 * (n * n + n + 3) / (9.0 * n * (n - 1))
    c1 = b1 - 1.0 / a1
    c2 = b2 - (n + 2) / (a1 * n) + a2 / (a1 * a1)
    e1 = c1 / a1
    e2 = c2 / (a1 * a1 + a2)
    var = e1 * S + e2 * S * (S - 1)
    if not var > 0.0:
        return None
    pi = 2.0 * float(int(ar_sum)) / (n * (n - 1))
    return (pi - S / a1) / math.sqrt(var)


def _filter_mask(packed, lo, hi, cfg):
    """SNPs of [lo, hi) that pass the position and variant_type filters of ``cfg`` (a ScanConfig: ann_want; or
    an object with ``variant_type``)."""
    m = np.ones(hi - lo, bool)
    pos = packed.pos[lo:hi].astype(np.int64)
    start, end = getattr(cfg, "start_position", None), getattr(cfg, "end_position", None)
    if start is not None:
        m &= pos >= int(start)
    if end is not None:
        m &= pos <= int(end)
    if hasattr(cfg, "ann_want"):
        if int(cfg.ann_want) >= 0:
            m &= packed.ann_id[lo:hi] == int(cfg.ann_want)
    elif getattr(cfg, "variant_type", None) is not None:
        m &= packed.variant_mask(cfg.variant_type)[lo:hi].astype(bool)
    return m


def window_sums(packed, begin, end, cfg) -> np.ndarray:
    """The host twin of k_div_win: DIVERSITY_DTYPE sums of the windows [begin[i], end[i]) of ``packed`` under
    ``cfg`` (n1p, n2p, the filters).  ``begin`` / ``end``: scalars or equal-length sequences."""
    begin = np.atleast_1d(np.asarray(begin, np.int64))
    end = np.atleast_1d(np.asarray(end, np.int64))
    out = np.zeros(len(begin), L.DIVERSITY_DTYPE)
    nfull = (2 * int(cfg.n1p), 2 * int(cfg.n2p))
    for i, (lo, hi) in enumerate(zip(begin.tolist(), end.tolist())):
        if hi <= lo:
            continue
        m = _filter_mask(packed, lo, hi, cfg)
        c = packed.counts[lo:hi][m]
        r = [((c >> np.uint32(s)) & np.uint32(0xFF)).astype(np.int64) for s in (0, 8, 16, 24)]
        r1, a1, r2, a2 = r
        o = out[i]
        for k, (rr, aa) in enumerate(((r1, a1), (r2, a2)), start=1):
            n = rr + aa
            ar = aa * rr
            ok = n >= 2
            den = np.where(ok, n * (n - 1), 1).astype(np.float64)
            o[f"pi{k}"] = math.fsum(np.where(ok, 2.0 * ar / den, 0.0).tolist())
            seg = ok & (aa > 0) & (aa < n)
            o[f"s{k}"] = int(seg.sum())
            o[f"thw{k}"] = math.fsum((1.0 / _H[n[seg]]).tolist())
            full = n == nfull[k - 1]
            o[f"s{k}_full"] = int((seg & full).sum())
            o[f"ar{k}_full"] = int(ar[full].sum())
        n1, n2 = r1 + a1, r2 + a2
        ok = (n1 >= 1) & (n2 >= 1)
        den = np.where(ok, n1 * n2, 1).astype(np.float64)
        o["dxy"] = math.fsum(np.where(ok, (a1 * r2 + r1 * a2) / den, 0.0).tolist())
        out[i] = o
    return out


def _kind(mode):
    if mode in ("bp", "snps"):
        return mode
    if mode == L.WINDOW_BP:
        return "bp"
    if mode == L.WINDOW_SNPS:
        return "snps"
    raise ValueError(f"mode must be 'bp' or 'snps' (or L.WINDOW_BP / L.WINDOW_SNPS), got {mode!r}")


def rows(recs, div, packed, window, mode, step=None, pop_sizes=None, regions=None) -> dict:
    """{window label: the twelve KEYS} from a plan's window records ``recs`` and its diversity records ``div``
    (same index), labels as the scans make them (post.record_labels: ``mode`` "bp" with ``window`` bp, sliding by
    ``step``; or "snps" with ``window`` SNPs per window).  Records that are no window (empty slots, the Q9 helper, an
    S-SNP window without 2D SFS entries) give no row.  pi, dxy, da = dxy - (pi1 + pi2) / 2 and theta_W are per
    site (module docstring); S, S_full and Tajima's D are not scaled.  ``pop_sizes`` = (pop1_size, pop2_size)
    diploid individuals: Tajima's D is formed from the SNPs fully called in the population (n = 2 pop_size); without
    it the two tajima_d columns are None.  ``regions`` (the Regions of a regions plan; ``window`` / ``mode`` /
    ``step`` unused): the keys are the regions' row keys, the per-site divisor each region's own length
    ``last - first + 1``, and an empty region has a row of twelve None (post.region_scan gives it a row too)."""
    if len(recs) != len(div):
        raise ValueError("window records and diversity records differ in length")
    spans = None
    if regions is not None:
        kind = "regions"
        labels = post.region_labels(recs, regions)
        spans = regions.lengths()
    else:
        kind = _kind(mode)
        labels = post.record_labels(recs, packed, kind, int(window), step)
    out = {}
    for i, (r, d, lb) in enumerate(zip(recs, div, labels)):
        if lb is None:
            continue
        if spans is not None:
            span = float(int(spans[i]))
        elif kind == "bp":
            span = float(int(window))
        else:
            span = float(int(packed.pos[int(r["end"]) - 1]) - int(packed.pos[int(r["begin"])]) + 1)
        pi1, pi2, dxy = float(d["pi1"]) / span, float(d["pi2"]) / span, float(d["dxy"]) / span
        row = {"pi_pop1": pi1, "pi_pop2": pi2, "dxy": dxy, "da": dxy - (pi1 + pi2) / 2,
               "theta_w_pop1": float(d["thw1"]) / span, "theta_w_pop2": float(d["thw2"]) / span,
               "S_pop1": int(d["s1"]), "S_pop2": int(d["s2"]),
               "S_full_pop1": int(d["s1_full"]), "S_full_pop2": int(d["s2_full"]),
               "tajima_d_pop1": None, "tajima_d_pop2": None}
        if pop_sizes is not None:
            row["tajima_d_pop1"] = tajima_d(2 * int(pop_sizes[0]), d["s1_full"], d["ar1_full"])
            row["tajima_d_pop2"] = tajima_d(2 * int(pop_sizes[1]), d["s2_full"], d["ar2_full"])
        out[lb] = row
    if regions is not None:
        for r, k in zip(recs, regions.slot_keys()):
            if r["flags"] & L.W_EMPTY:
                out[k] = dict.fromkeys(KEYS)
    return out


def add_columns(stats, recs, div, packed, window, mode, step=None, pop_sizes=None, regions=None):
    """Add the twelve KEYS to every row of a scan's result dict ``stats`` (the rows of ``recs``' windows)."""
    dv = rows(recs, div, packed, window, mode, step, pop_sizes, regions)
    for lb, row in stats.items():
        row.update(dv[lb])
    return stats
