"""Test-only: fixtures, references and tolerances of the projected-scan tests (test_project_scan_cpu.py,
test_project_scan_gpu.py).

The genome (``genome``) is project_util's (chromosomes of 1 .. 9,000 SNPs, pop 18 / 14, 2 % missing alleles, the
projection's awkward SNPs planted) with three consecutive ``*_below`` SNPs planted on a 3-SNP window of the last
chromosome (``ALL_DROPPED``): a window whose members are all dropped.

Two references:

* ``closed_form``: the statistic's closed form in float64 on the host from grids that ``Plan.project`` returned (the
  same rounded terms the scan kernel sums), with the scale ``A = sum |x_k ln(x_k / N)| + |x_k lp_k|`` its rounding
  acts on -- checks the device's arithmetic alone, tolerance 1e-10 A;
* ``twin``: sfs2d.spectra.project_scan_np with exact weights, shared per call signature -- checks everything, within
  ``bounds``: the first-order effect of the fixed point and of the weights' error on T.  A window bin x_k is off by at
  most d_k = f K 2^-(e + 1) + 2 R x_k (K used SNPs, one rounding per term, f = 2 on a folded grid whose bin is two
  unfolded ones; R = project_util.R()), a background bin by d'_k from K_c and e_bg.  dT/dx_k = 2 (ln(x_k / N) - lp_k)
  (the derivative through N cancels: sum x_k / N = 1) and dT/db_k = 2 (N / B - x_k / b_k), so
  |dT| <= 2 sum_k |ln(x_k / N) - lp_k| d_k + 2 sum_k |N / B - x_k / b_k| d'_k to first order; the tests allow twice
  that (the second-order terms) plus 1e-10 A.  A bin of a folded 1D marginal sums the 2 (m_other + 1) unfolded bins of
  two rows (or columns), so its d is 2 (m_other + 1) K 2^-(e + 1) + 2 R x_k."""
import math

import numpy as np

import project_util as PU
from sfs2d import _lib as L
from sfs2d import spectra as SP

_DATA, _TWIN = {}, {}
ALL_DROPPED = 300      # offset of the all-dropped 3-SNP window in the last chromosome (a multiple of 3)


def genome(n1p, n2p, m, lengths=None, full=False):
    key = (n1p, n2p, m, None if lengths is None else tuple(lengths), full)
    if key in _DATA:
        return _DATA[key]
    from sfs2d.pack import PackedSNPs, pack_counts
    p = PU.genome(n1p, n2p, m, lengths=lengths, full=full)
    r = [p.ref1.astype(np.int64), p.alt1.astype(np.int64), p.ref2.astype(np.int64), p.alt2.astype(np.int64)]
    kinds = PU.planted(n1p, n2p, *m)
    at = int(p.chrom_off[-2]) + ALL_DROPPED
    if at + 3 <= p.n:
        for i, kind in enumerate(("p1_below", "p2_below", "both_below")):
            for f, v in zip(r, kinds[kind]):
                f[at + i] = v
    q = PackedSNPs(pack_counts(*r), p.pos, p.chrom_off, p.chrom_names, p.ann_id, p.ann_names)
    _DATA[key] = q
    return q


def records(p, size=None):
    """Window records as a plan would write them, as far as the twin reads them: whole chromosomes (``size`` None)
    or SNP-count windows of ``size`` SNPs (the incomplete tail of a chromosome dropped)."""
    out = []
    for c in range(p.nchrom):
        lo, hi = int(p.chrom_off[c]), int(p.chrom_off[c + 1])
        if size is None:
            out.append((c, 0, lo, hi))
        else:
            out.extend((c, k, lo + k * size, lo + (k + 1) * size) for k in range((hi - lo) // size))
    recs = np.zeros(len(out), L.WINDOW_DTYPE)
    for i, (c, k, b, e) in enumerate(out):
        recs[i]["chrom"], recs[i]["wid"], recs[i]["begin"], recs[i]["end"] = c, k, b, e
    recs["snp_count"] = recs["end"] - recs["begin"]
    return recs


def twin(p, recs, cfg, m1, m2, bg_chrom=None):
    """project_scan_np with exact weights, computed once per call signature and shared (read-only)."""
    key = (id(p), recs[["chrom", "begin", "end", "flags"]].tobytes(), cfg.n1p, cfg.n2p, bool(cfg.fold), int(cfg.ann_want),
           cfg.start_position, cfg.end_position, m1, m2, bg_chrom)
    if key not in _TWIN:
        out = SP.project_scan_np(p, recs, cfg, m1, m2, bg_chrom, exact=True)
        out.setflags(write=False)
        _TWIN[key] = out
    return _TWIN[key]


def _inner(m):
    return [j for j in range(1, m + 1) if 2 * j < m]


def spectra_of(grid, fold):
    """(inner 2D bins, folded pop-1 marginal at its inner bins, pop-2 likewise) of one unfolded projected grid."""
    g = SP.fold_projected(grid) if fold else np.asarray(grid)
    s1, s2 = SP.projected_marginals(g)
    m1, m2 = g.shape[0] - 1, g.shape[1] - 1
    return g.ravel()[1:-1], SP.fold1d_projected(s1)[_inner(m1)], SP.fold1d_projected(s2)[_inner(m2)]


def _form(x, b, dx=None, db=None):
    """(T, A, first-order bound) of one spectrum x against b (float64 arrays)."""
    N, B = math.fsum(x.tolist()), math.fsum(b.tolist())
    if N == 0 or B == 0:
        return math.nan, 0.0, 0.0
    hit = x > 0
    if (b[hit] == 0).any():
        return math.inf, 0.0, 0.0
    lx, lp = np.log(x[hit] / N), np.log(b[hit] / B)
    T = 2.0 * math.fsum((x[hit] * (lx - lp)).tolist())
    A = math.fsum((np.abs(x[hit] * lx) + np.abs(x[hit] * lp)).tolist())
    bound = 0.0
    if dx is not None:
        pos = b > 0
        bound = 2.0 * math.fsum((np.abs(lx - lp) * dx[hit]).tolist()) + \
            2.0 * math.fsum((np.abs(N / B - x[pos] / b[pos]) * db[pos]).tolist())
    return T, A, bound


def closed_form(grid, bg_grid, fold, K=None, Kc=None, e=None, e_bg=None):
    """Per statistic (t2d, t1d_p1, t1d_p2): (T, A, bound) from one window's and its background's unfolded grids.
    With K, Kc, e, e_bg: the first-order bound of the module docstring, else 0."""
    m1, m2 = grid.shape[0] - 1, grid.shape[1] - 1
    xs, bs = spectra_of(grid, fold), spectra_of(bg_grid, fold)
    out = []
    for i, (x, b) in enumerate(zip(xs, bs)):
        dx = db = None
        if K is not None:
            f = (2 if fold else 1) if i == 0 else 2 * ((m2, m1)[i - 1] + 1)
            r = PU.R()
            dx = f * K * math.ldexp(1.0, -(e + 1)) + 2.0 * r * x
            db = f * Kc * math.ldexp(1.0, -(e_bg + 1)) + 2.0 * r * b
        out.append(_form(np.asarray(x, np.float64), np.asarray(b, np.float64), dx, db))
    return out


def fixed_sums(grid, fold, e):
    """(N2, N1a, N1b) of one unfolded grid of ``Plan.project`` as Python integers at the fixed point 2^-e (every
    word of the grid is an integer below 2^53 there; the sums are taken on Python integers)."""
    scaled = np.ldexp(np.asarray(grid, np.float64), e)
    assert np.array_equal(scaled, np.rint(scaled)) and scaled.max(initial=0.0) < 2.0 ** 53
    ints = np.empty(scaled.size, object)
    ints[:] = [int(v) for v in scaled.ravel().tolist()]
    return tuple(sum(x.tolist()) for x in spectra_of(ints.reshape(scaled.shape), fold))
