"""Test-only: fixtures, the exact reference and the tolerances of the projected-spectra tests (test_project_cpu.py,
test_project_gpu.py).

The genome (``genome``) is spectra_util's: chromosomes of 1, 63, 64, 65, 255, 256, 257, 2,047, 2,049 and 9,000 SNPs
with missing alleles at 2 % per allele.  Planted among the generated SNPs, at the row edges and every 41st SNP, are
the kinds that take the kernel's two branches (``planted``): called counts one below, at and one above the projection
in each population alone and in both, alt counts 0 and n, an over-called SNP and a tie of the joint fold.  The kinds
depend on the projection, so there is a genome per (pop sizes, projection).  ``full`` = True: a copy in which every
generated SNP is fully called (ref = 2 pop_size - alt).  ``assert_kinds`` asserts on the twin's output that the
fixture holds every kind; ``assert_dropped_share`` the condition that no whole chromosome of 255 SNPs or more loses
more than a quarter of its members.

The reference is sfs2d.spectra.project_np with exact rational weights; ``twin`` computes it once per (data,
configuration, projection, selection) and shares it -- treat the arrays as read-only.

Tolerances.  A weight from the ln k! table has a relative error bounded by R = 4 x the worst error that
``weights_error`` measures on the host over the cases of test_project_cpu.py (every (n, a, m) with n <= 72 and a
seeded sample of 20,000 with n up to 510).  A grid bin is a sum of K_g or fewer terms (K_g: the group's used SNPs),
each the product of two weights (relative error 2 R) rounded to nearest once at 2^-e (absolute error 2^-(e + 1)):
|got - exact| <= K_g 2^-(e + 1) + 2 R exact (``assert_grids``)."""
import math

import numpy as np

import spectra_util as SU
from sfs2d import _lib as L
from sfs2d import spectra as SP

_DATA, _TWIN, _R = {}, {}, []


def planted(n1p, n2p, m1, m2):
    """(ref1, alt1, ref2, alt2) by kind; every count <= 255, every key inside the grid, every one a member."""
    N1, N2 = 2 * n1p, 2 * n2p

    def c(n, a):
        return (n - a, a)
    mid1, mid2 = c(N1, N1 // 3), c(N2, N2 // 3)       # fully called, alt sum below the fold
    return {
        "p1_below": c(m1 - 1, 1) + mid2,                     # n1 = m1 - 1: dropped
        "p1_at": c(m1, m1 // 2) + mid2,                      # n1 = m1: one bin in population 1
        "p1_above": c(m1 + 1, (m1 + 1) // 2) + mid2,         # n1 = m1 + 1: two bins
        "p2_below": mid1 + c(m2 - 1, 1),
        "p2_at": mid1 + c(m2, m2 // 2),
        "p2_above": mid1 + c(m2 + 1, (m2 + 1) // 2),
        "both_below": c(m1 - 1, 1) + c(m2 - 1, 1),
        "both_at": c(m1, m1 // 2) + c(m2, m2 // 2),
        "both_above": c(m1 + 1, (m1 + 1) // 2) + c(m2 + 1, (m2 + 1) // 2),
        "a_zero": c(N1, 0) + c(N2, 3),                       # a1 = 0: population 1 in bin 0 alone
        "a_full": c(N1, N1) + mid2,                          # a1 = n1: population 1 in bin m1 alone
        "over_called": c(N1 + 2, 5) + c(N2 + 1, 2),          # n_k > 2 pop_size: used like any other
        "fold_tie": c(N1, n1p + 3) + c(N2, n2p - 3),         # alt1 + alt2 == n1p + n2p: the scan does not fold it
    }


def genome(n1p, n2p, m=None, lengths=None, full=False):
    """``m`` None: nothing planted (the generated SNPs alone)."""
    lengths = SU.LENGTHS if lengths is None else list(lengths)
    key = (n1p, n2p, m, tuple(lengths), full)
    if key in _DATA:
        return _DATA[key]
    from sfs2d.pack import PackedSNPs, pack_counts
    p = SU.genome(n1p, n2p, lengths, plant=False)
    r = [p.ref1.astype(np.int64), p.alt1.astype(np.int64), p.ref2.astype(np.int64), p.alt2.astype(np.int64)]
    if full:
        r[0], r[2] = 2 * n1p - r[1], 2 * n2p - r[3]
    if m is not None:
        kinds = list(planted(n1p, n2p, *m).values())
        big = int(p.chrom_off[-2])   # the last chromosome's first SNP
        at = sorted(set(list(range(5, p.n, 41)) + [big + x for x in (0, 63, 64, 255, 256, 257, 1023, 1024, 1025)
                                                   if big + x < p.n] + [p.n - 1]))
        for k, i in enumerate(at):
            for f, v in zip(r, kinds[k % len(kinds)]):
                f[i] = v
    assert max(int(x.max()) for x in r) <= 255 and min(int(x.min()) for x in r) >= 0
    q = PackedSNPs(pack_counts(*r), p.pos, p.chrom_off, p.chrom_names, p.ann_id, p.ann_names)
    _DATA[key] = q
    return q


class Cfg:
    """The part of a configuration the twin reads."""

    def __init__(self, n1p, n2p, fold=True, ann_want=-1, start_position=None, end_position=None):
        self.n1p, self.n2p, self.fold, self.ann_want = n1p, n2p, fold, ann_want
        self.start_position, self.end_position = start_position, end_position


def _one(p, i, cfg, m1, m2):
    recs = np.zeros(1, L.WINDOW_DTYPE)
    recs["begin"], recs["end"] = i, i + 1
    g, u, d = SP.project_np(p, recs, cfg, m1, m2, exact=True)
    return g[0], int(u[0]), int(d[0])


def assert_kinds(p, n1p, n2p, m1, m2, missing=True):
    """The fixture's properties, on the twin's output (``missing`` False: the fully called copy)."""
    cfg = Cfg(n1p, n2p)
    kinds = planted(n1p, n2p, m1, m2)
    r1, a1, r2, a2 = (x.astype(np.int64) for x in (p.ref1, p.alt1, p.ref2, p.alt2))

    def where(kind):
        v = kinds[kind]
        i = np.nonzero((r1 == v[0]) & (a1 == v[1]) & (r2 == v[2]) & (a2 == v[3]))[0]
        assert i.size, kind
        return int(i[0])

    def support(g):
        nz = np.array([[x != 0 for x in row] for row in g])
        return int(nz.any(axis=1).sum()), int(nz.any(axis=0).sum())
    for kind in ("p1_below", "p2_below", "both_below"):
        g, u, d = _one(p, where(kind), cfg, m1, m2)
        assert (u, d) == (0, 1) and not g.any(), kind
    for kind, sup in (("p1_at", (1, None)), ("p2_at", (None, 1)), ("both_at", (1, 1)), ("p1_above", (2, None)),
                      ("p2_above", (None, 2)), ("both_above", (2, 2))):
        g, u, d = _one(p, where(kind), cfg, m1, m2)
        assert (u, d) == (1, 0) and g.sum() == 1, kind
        got = support(g)
        assert all(s is None or s == t for s, t in zip(sup, got)), (kind, got)
    i = where("both_at")
    assert _one(p, i, cfg, m1, m2)[0][a1[i], a2[i]] == 1                     # n == m: the indicator of (a1, a2)
    g = _one(p, where("a_zero"), cfg, m1, m2)[0]
    assert g[0].sum() == 1                                                   # a1 = 0: row 0 alone
    g = _one(p, where("a_full"), cfg, m1, m2)[0]
    assert g[m1].sum() == 1                                                  # a1 = n1: row m1 alone
    i = where("over_called")
    assert r1[i] + a1[i] > 2 * n1p and r2[i] + a2[i] > 2 * n2p and _one(p, i, cfg, m1, m2)[1:] == (1, 0)
    i = where("fold_tie")
    assert a1[i] + a2[i] == n1p + n2p and _one(p, i, cfg, m1, m2)[1:] == (1, 0)
    nc1, nc2 = r1 + a1, r2 + a2
    if missing:      # missing calls among the generated SNPs: a fifth of them at least, in either population
        assert 5 * int((nc1 < 2 * n1p).sum()) > p.n and 5 * int((nc2 < 2 * n2p).sum()) > p.n


def assert_dropped_share(p, cfg, m1, m2):
    """No whole chromosome of 255 SNPs or more loses more than 25 % of its members to the projection."""
    g, used, dropped = twin(p, None, cfg, m1, m2, rec=[-(c + 1) for c in range(p.nchrom)])
    seen = 0
    for c in range(p.nchrom):
        if int(p.chrom_off[c + 1] - p.chrom_off[c]) < 255:
            continue
        n = int(used[c] + dropped[c])
        assert n > 0 and 4 * int(dropped[c]) <= n, (c, int(dropped[c]), n)
        seen += 1
    assert seen >= 3


def twin(p, recs, cfg, m1, m2, rec=None, grp=None, ngroups=None):
    """project_np (float grids, used, dropped), computed once per call signature and shared (read-only)."""
    recs = np.zeros(0, L.WINDOW_DTYPE) if recs is None else recs
    key = (id(p), recs[["begin", "end", "flags"]].tobytes(), cfg.n1p, cfg.n2p, bool(cfg.fold), int(cfg.ann_want),
           cfg.start_position, cfg.end_position, m1, m2, None if rec is None else tuple(np.asarray(rec).tolist()),
           None if grp is None else tuple(np.asarray(grp).tolist()), ngroups)
    if key not in _TWIN:
        out = SP.project_np(p, recs, cfg, m1, m2, rec, grp, ngroups)
        for a in out:
            a.setflags(write=False)
        _TWIN[key] = out
    return _TWIN[key]


# ------------------------------------------------------------------------------------------------- tolerances

def _exact_rows(n, a, m, C):
    den = C[n][m]
    return [C[a][j] * C[n - a][m - j] / den if 0 <= m - j <= n - a and j <= a else 0.0 for j in range(m + 1)]


def weight_cases():
    """Every (n, a, m) with n <= 72, then a seeded sample of 20,000 with n up to 510."""
    for n in range(73):
        for a in range(n + 1):
            for m in range(n + 1):
                yield n, a, m
    rng = np.random.default_rng(510)
    n = rng.integers(1, 511, 20000)
    a = (rng.random(20000) * (n + 1)).astype(np.int64)
    m = (rng.random(20000) * (n + 1)).astype(np.int64)
    yield from zip(n.tolist(), a.tolist(), m.tolist())


def weights_error(cases, check=None):
    """The worst relative error of sfs2d_project_weights over the weights above 1e-30 of ``cases``, against exact
    rationals (integer binomials, one correctly rounded division).  ``check(n, a, m, got, exact)``: called per
    case."""
    import ctypes as C
    lib = L.lib()
    comb = [[math.comb(n, k) for k in range(n + 1)] for n in range(511)]
    worst = 0.0
    buf = np.zeros(512, np.float64)
    ptr = buf.ctypes.data_as(C.c_void_p)
    for n, a, m in cases:
        assert lib.sfs2d_project_weights(n, a, m, ptr) == 0, (n, a, m)
        got = buf[:m + 1]
        want = np.array(_exact_rows(n, a, m, comb), np.float64)
        if check is not None:
            check(n, a, m, got, want)
        big = want > 1e-30
        if big.any():
            worst = max(worst, float(np.max(np.abs(got[big] - want[big]) / want[big])))
    return worst


def R():
    """4 x the worst relative error of a weight (measured once per session)."""
    if not _R:
        _R.append(4.0 * weights_error(weight_cases()))
    return _R[0]


def assert_grids(got, used, dropped, want, e, what=""):
    """(grids, used, dropped) of Plan.project against the twin's: the counts exact, every bin within
    K_g 2^-(e + 1) + 2 R value, the grid's sum n_used within the bound summed over its bins."""
    wg, wu, wd = want
    assert got.dtype == np.float64 and got.shape == wg.shape, (what, got.shape, wg.shape)
    assert np.array_equal(used, wu) and np.array_equal(dropped, wd), (what, used.tolist()[:8], wu.tolist()[:8])
    r = R()
    step = math.ldexp(1.0, -(e + 1))
    for g in range(len(wg)):
        tol = int(wu[g]) * step + 2.0 * r * wg[g]
        err = np.abs(got[g] - wg[g])
        if not (err <= tol).all():
            k = np.unravel_index(np.argmax(err - tol), err.shape)
            raise AssertionError((what, "group", g, "bin", k, float(got[g][k]), float(wg[g][k]), float(tol[k])))
        assert abs(math.fsum(got[g].ravel().tolist()) - int(wu[g])) <= math.fsum(tol.ravel().tolist()), (what, g)
    # every word a multiple of 2^-e
    assert np.array_equal(np.ldexp(got, e), np.rint(np.ldexp(got, e))), what


def fixed_point_e(max_entries, per_entry):
    """e = min(40, 62 - bitlen(B)), B = the most entries of one group x the bound on one entry's SNPs."""
    return min(40, 62 - (max(1, int(max_entries)) * int(per_entry)).bit_length())


def assert_folded(got, want_unfolded, used, e, fold, what=""):
    """Grids as the class returns them (folded when ``fold``) against the twin's unfolded grids.  The fold is
    linear: a folded bin is the sum of two unfolded bins, so its bound is the sum of theirs, at most
    2 K_g 2^-(e + 1) + 2 R value; an unfolded grid keeps assert_grids' bound.  ``e``: the call's, or a lower bound
    of it (a larger e only tightens the true error)."""
    want = SP.fold_projected(want_unfolded) if fold else np.asarray(want_unfolded)
    k = np.asarray(used, np.float64).reshape((-1,) + (1,) * (want.ndim - 1))
    tol = (2 if fold else 1) * k * math.ldexp(1.0, -(e + 1)) + 2.0 * R() * want
    assert got.shape == want.shape and (np.abs(got - want) <= tol).all(), (what, float(np.abs(got - want).max()))
