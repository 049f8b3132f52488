"""Test-only: the diversity sums (include/sfs2d.h, sfs2d_diversity) straight from their definitions, in numpy, over
a PackedSNPs and a list of SNP ranges -- written apart from sfs2d.diversity.window_sums, which test_diversity_cpu
compares with it.  Every SNP that passes the position / variant_type filters takes part, the ones the 2D SFS
drops as bin (0, 0) included (their terms are 0 by the definitions, not by being skipped)."""
import math

import numpy as np

import golden_util as gu
from sfs2d import _lib as L

INTS = ("ar1_full", "ar2_full", "s1", "s2", "s1_full", "s2_full", "flags", "reserved")
DOUBLES = ("pi1", "pi2", "dxy", "thw1", "thw2")


def h(n):
    return sum(1.0 / i for i in range(1, int(n)))


def snp_terms(r1, a1, r2, a2, n1p, n2p):
    """One SNP's terms as Python numbers: dict of the record's fields."""
    t = {}
    for k, (r, a, npop) in enumerate(((r1, a1, n1p), (r2, a2, n2p)), start=1):
        n = r + a
        seg = n >= 2 and 0 < a < n
        t[f"pi{k}"] = 2 * a * r / (n * (n - 1)) if n >= 2 else 0.0
        t[f"s{k}"] = int(seg)
        t[f"thw{k}"] = 1.0 / h(n) if seg else 0.0
        full = n == 2 * npop
        t[f"s{k}_full"] = int(seg and full)
        t[f"ar{k}_full"] = a * r if full else 0
    n1, n2 = r1 + a1, r2 + a2
    t["dxy"] = (a1 * r2 + r1 * a2) / (n1 * n2) if n1 >= 1 and n2 >= 1 else 0.0
    return t


def passing(p, cfg):
    """Boolean per SNP: passes cfg's position and variant_type filters (cfg: oracle.Cfg)."""
    m = np.ones(p.n, bool)
    pos = p.pos.astype(np.int64)
    if cfg.start_position is not None:
        m &= pos >= cfg.start_position
    if cfg.end_position is not None:
        m &= pos <= cfg.end_position
    vm = p.variant_mask(cfg.variant_type)
    if vm is not None:
        m &= vm.astype(bool)
    return m


def expected(p, ranges, cfg):
    """DIVERSITY_DTYPE records of the SNP ranges [(begin, end)] (flags 0); cfg: oracle.Cfg."""
    ok = passing(p, cfg)
    hn = np.array([0.0, 0.0] + [h(n) for n in range(2, 512)])
    cols = {}
    r1, a1, r2, a2 = p.ref1, p.alt1, p.ref2, p.alt2
    for k, (r, a, npop) in enumerate(((r1, a1, cfg.n1p), (r2, a2, cfg.n2p)), start=1):
        n = r + a
        seg = ok & (n >= 2) & (a > 0) & (a < n)
        pi = np.zeros(p.n)
        two = ok & (n >= 2)
        pi[two] = 2.0 * (a[two] * r[two]) / (n[two] * (n[two] - 1))
        th = np.zeros(p.n)
        th[seg] = 1.0 / hn[n[seg]]
        full = ok & (n == 2 * npop)
        cols[f"pi{k}"], cols[f"thw{k}"] = pi, th
        cols[f"s{k}"], cols[f"s{k}_full"] = seg.astype(np.int64), (seg & full).astype(np.int64)
        cols[f"ar{k}_full"] = np.where(full, a * r, 0)
    n1, n2 = r1 + a1, r2 + a2
    both = ok & (n1 >= 1) & (n2 >= 1)
    dxy = np.zeros(p.n)
    dxy[both] = (a1[both] * r2[both] + r1[both] * a2[both]) / (n1[both] * n2[both])
    cols["dxy"] = dxy
    out = np.zeros(len(ranges), L.DIVERSITY_DTYPE)
    for i, (b, e) in enumerate(ranges):
        for f in DOUBLES:
            out[f][i] = math.fsum(cols[f][b:e].tolist())
        for f in INTS[:6]:
            out[f][i] = int(cols[f][b:e].sum())
    return out


def assert_records(got, want, what=""):
    """Integer fields exact; doubles within the project's 1e-10 relative, an expected 0.0 exactly 0.0."""
    assert len(got) == len(want), (what, len(got), len(want))
    for f in INTS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, (what, f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])
    for f in DOUBLES:
        for i in range(len(want)):
            assert gu.close(float(got[f][i]), float(want[f][i])), (what, f, i, got[f][i], want[f][i])


def expected_for_records(p, recs, cfg):
    """The records a plan's diversity call must give for its window records ``recs``: the sums of every
    record's own range, zero and flagged for empty slots and the Q9 helper."""
    dead = (recs["flags"] & (L.W_EMPTY | L.W_EXTRA)) != 0
    rng = [(0, 0) if d else (int(b), int(e)) for d, b, e in zip(dead, recs["begin"], recs["end"])]
    want = expected(p, rng, cfg)
    want["flags"] = recs["flags"] & (L.W_EMPTY | L.W_EXTRA)
    return want
