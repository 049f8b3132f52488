"""Test-only: the small genome, the region list and the oracle reference of the region-window tests
(test_regions_gpu.py).

The genome (``genome``; ~9,000 SNPs, scanned under SFS2D_TILE = 4096): chromosomes of 1 SNP (monomorphic: a None
window), 7 SNPs (it gets NO region), 3,001 SNPs with repeated positions and a SNP at position 0, no SNPs at all, and
6,000 SNPs with a gap of 14,400 bp.  Every 37th SNP carries one of Fst's edge values, as in the sliding tests.

The list (``items``; the caller's order, which mixes the chromosomes -- Regions sorts it stably) holds, by name:
empty regions before the first SNP, after the last SNP and between two neighbouring SNPs; ``first`` exactly on a
SNP, ``last`` exactly on a SNP, both on a repeated position; ``first == 0`` and ``last == 2^32 - 1``; a single-SNP
region; a whole-chromosome region of 6,000 SNPs (k_scan_w's streamed rows); nested and overlapping regions, an
identical pair (named apart), regions unsorted within their chromosome; a region on the SNP-less chromosome.

``reference`` builds, per slot, (chrom, wid, begin, end) with np.searchsorted from the definition (begin: the first
SNP of the chromosome with pos >= first, end: the first with pos >= last + 1) and the oracle's records and Fst of the
non-empty ones, once per configuration; ``check`` pins a record table and its Fst column to it: integers exact, T by
golden_util.close with None exactly where the oracle has None (sfs2d.post._v), Fst within 1e-12 + 1e-10 |x|."""
import numpy as np

import golden_util as gu
from oracle import sfs_oracle as O

LENGTHS = [1, 7, 3001, 0, 6000]
VT = "intron_variant"
INTS = ("chrom", "wid", "begin", "end", "snp_count", "n2", "n2_all", "n1a", "n1b", "flags")
POS_MAX = (1 << 32) - 1
GAP = (20001, 34401)   # no SNP of the last chromosome in [lo, hi)
_DATA, _REF, _RG = {}, {}, {}


def _positions(rng, n, lo, span, gap=None):
    free = np.arange(lo, span)
    if gap is not None:
        free = free[(free < gap[0]) | (free >= gap[1])]
    pos = rng.choice(free, size=n, replace=False)
    pos.sort()
    return pos


def genome(n1p, n2p):
    key = (n1p, n2p)
    if key in _DATA:
        return _DATA[key]
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(160 + n1p))
    n1, n2 = 2 * n1p, 2 * n2p
    # chromosome 2: 2,990 distinct positions in [3, 16000), five of them three times (+ 10), and position 0
    d2 = _positions(rng, 2990, 3, 16000)
    rep = d2[[40, 41, 700, 1500, 2989]]   # (two neighbours, and the chromosome's last position)
    p2 = np.sort(np.concatenate([[0], d2, rep, rep]))
    pos = [np.array([50]), np.array([0, 1, 1600, 1601, 6400, 6401, 12800]), p2, np.zeros(0, np.int64),
           _positions(rng, LENGTHS[4], 5, 64000, GAP)]
    assert [len(x) for x in pos] == LENGTHS
    counts, ann = [], []
    for x in pos:
        _, r1, a1, r2, a2 = synth_chrom(rng, len(x), n1p, n2p)
        counts.append(pack_counts(r1, a1, r2, a2))
        ann.append(rng.integers(0, 3, size=len(x)).astype(np.uint16))
    counts = np.concatenate(counts)
    counts[0] = int(pack_counts(np.array([n1]), np.array([0]), np.array([n2]), np.array([0]))[0])   # monomorphic
    h1, h2 = n1 // 2, n2 // 2
    edge = [(n1, 0, n2 - 1, 1), (n1 - 1, 1, n2, 0), (0, n1, h2, n2 - h2), (h1, n1 - h1, 0, n2), (0, n1, n2 - 1, 1),
            (n1, 0, 0, n2), (0, n1, n2, 0), (1, 1, h2, h2), (0, 2, h2 + 3, h2 - 3), (2, 0, 1, 1),
            (1, 0, h2, h2), (0, 1, h2, h2), (h1, h1, 0, 1), (0, 0, h2, h2), (h1, h1, 0, 0), (0, 1, 0, 1)]
    at = np.arange(11, len(counts), 37)
    e = np.array([edge[k % len(edge)] for k in range(len(at))])
    counts[at] = pack_counts(e[:, 0], e[:, 1], e[:, 2], e[:, 3])
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    p = PackedSNPs(counts, np.concatenate(pos).astype(np.uint32), off, [f"chr{i:04d}" for i in range(len(LENGTHS))],
                   np.concatenate(ann), ["intergenic_region", VT, "missense_variant"], "p1", "p2")
    _DATA[key] = p
    return p


def items(p):
    """The region list, (chrom_name, first, last, name) in the caller's order."""
    P2 = p.pos[int(p.chrom_off[2]):int(p.chrom_off[3])].astype(np.int64)
    P4 = p.pos[int(p.chrom_off[4]):int(p.chrom_off[5])].astype(np.int64)
    u, n = np.unique(P2, return_counts=True)
    rep = u[n > 1]
    assert len(rep) == 5 and P2[0] == 0 and P4[0] > 1
    i = 200 + int(np.argmax(np.diff(P4[200:]) >= 2))   # two neighbouring SNPs with a site between them
    c0, c2, c3, c4 = (p.chrom_names[c] for c in (0, 2, 3, 4))
    return [
        (c4, 1, int(P4[0]) - 1, "before_first"),                  # empty
        (c2, int(rep[0]), int(rep[2]), "repeat_to_repeat"),       # first and last on repeated positions
        (c4, int(P4[100]), int(P4[100]), "single_snp"),
        (c4, int(P4[i]) + 1, int(P4[i + 1]) - 1, "between_neighbours"),   # empty, in mid-list
        (c4, 0, POS_MAX, "whole_chrom4"),                         # first == 0, last == 2^32 - 1, 6,000 SNPs
        (c2, 0, 0, "pos0_only"),                                  # first == 0: the SNP at position 0 alone
        (c2, 1, 9000, "from_1_without_pos0"),                     # first == 1: not the SNP at position 0
        (c3, 1, 1000, "snpless_chrom"),                           # empty: the chromosome holds no SNP
        (c4, int(P4[-1]) + 1, int(P4[-1]) + 500, "after_last"),   # empty
        (c4, 10000, 40000, "outer"),                              # holds the gap
        (c4, 12000, 13000, "nested"),
        (c4, 36000, 45000, "overlapping"),
        (c4, 40000, 47000, "dupA"),
        (c4, 40000, 47000, "dupB"),                               # an identical pair
        (c4, int(P4[300]), int(P4[900]), "snp_to_snp"),           # first and last exactly on SNPs
        (c0, 1, 100, "monomorphic"),                              # a None window
        (c2, int(rep[4]), int(rep[4]), "last_repeat"),            # the chromosome's last position, three SNPs
        (c2, int(P2[50]), int(P2[50]) + 3000, "from_snp"),
        (c4, POS_MAX - 9, POS_MAX, "far_right"),                  # empty, last == 2^32 - 1
        (c2, int(rep[1]) + 1, int(rep[2]) - 1, "open_between_repeats"),
    ]


def regions(p):
    from sfs2d.regions import Regions
    if id(p) not in _RG:
        _RG[id(p)] = Regions(p.chrom_names, items(p))
    return _RG[id(p)]


def slots_of(p, rg):
    """[(chrom, wid, begin, end)] per slot from the definition; begin == end: an empty region."""
    out, seen = [], {}
    for c, f, l in zip(rg.chrom.tolist(), rg.first.tolist(), rg.last.tolist()):
        lo, hi = int(p.chrom_off[c]), int(p.chrom_off[c + 1])
        pos = p.pos[lo:hi].astype(np.int64)
        b = lo + int(np.searchsorted(pos, f, "left"))
        e = lo + int(np.searchsorted(pos, l + 1, "left"))
        out.append((c, seen.get(c, 0), b, e))
        seen[c] = seen.get(c, 0) + 1
    return out


def no_cancelled_t(values):
    """No oracle T in (0, 1e-2): below that the absolute rounding error of any evaluation order passes 1e-10
    relative."""
    for v in values:
        assert v is None or v == 0.0 or not np.isfinite(v) or abs(v) >= 1e-2, v


def oracle_of(p, slots, ocfg, bg_chrom=None):
    """(slots, oracle records of the non-empty ones, their Fst)."""
    bgs = O.chrom_backgrounds(p, ocfg)
    wins = [x for x in slots if x[2] < x[3]]
    recs = O.window_records(p, wins, ocfg, (lambda c: bgs[c]) if bg_chrom is None else (lambda c: bgs[bg_chrom]))
    fst = [O.window_fst(p, np.arange(x[2], x[3]), ocfg) for x in wins]
    return slots, recs, fst


def reference(n1p, n2p, vt=None, fold=True, start=None, bg_chrom=None):
    """The reference of the small genome's list, once per case, with the fixture's properties asserted on it."""
    key = (n1p, n2p, vt, fold, start, bg_chrom)
    if key not in _REF:
        p = genome(n1p, n2p)
        rg = regions(p)
        slots = slots_of(p, rg)
        ref = oracle_of(p, slots, O.Cfg(n1p, n2p, vt, fold, start, None), bg_chrom)
        _, recs, _ = ref
        no_cancelled_t(o[t] for o in recs for t in ("T2D", "T1D_p1", "T1D_p2"))
        assert any(o["T2D"] is None for o in recs)
        assert any(o["T2D"] is not None and np.isfinite(o["T2D"]) for o in recs)
        assert max(x[3] - x[2] for x in slots) > 512
        assert any(x[2] == x[3] for x in slots[1:-1])   # an empty slot in mid-list
        _REF[key] = ref
    return _REF[key]


def check(recs, fst, ref):
    from sfs2d import _lib as L
    from sfs2d import post
    slots, orec, ofst = ref
    assert len(recs) == len(slots), (len(recs), len(slots))
    assert fst is None or len(fst) == len(slots)
    k = 0
    for i, ((c, j, b, e), r) in enumerate(zip(slots, recs)):
        assert (int(r["chrom"]), int(r["wid"])) == (c, j), (i, c, j, int(r["chrom"]), int(r["wid"]))
        if b == e:
            assert int(r["flags"]) & L.W_EMPTY and (int(r["begin"]), int(r["end"])) == (0, 0), (i, c, j)
            assert fst is None or np.isnan(fst[i]), (i, "fst of an empty slot")
            continue
        o = orec[k]
        assert not int(r["flags"]) & L.W_EMPTY and (int(r["begin"]), int(r["end"])) == (b, e), (i, c, j, b, e)
        for a, q in (("snp_count", "snp_count"), ("n2", "N2"), ("n2_all", "N2_all"), ("n1a", "N1a"), ("n1b", "N1b")):
            assert int(r[a]) == o[q], (i, a, int(r[a]), o[q])
        for which, q in ((2, "T2D"), (1, "T1D_p1"), (0, "T1D_p2")):
            v = post._v(r, which)
            assert (v is None) == (o[q] is None), (i, q, v, o[q])
            assert gu.close(v, o[q]), (i, q, v, o[q])
        if fst is not None:
            g, f = float(fst[i]), ofst[k]
            assert (np.isnan(g) if f is None else abs(g - f) <= 1e-12 + 1e-10 * abs(f)), (i, "fst", g, f)
        k += 1
    assert k == len(orec)


def same_ints(a, b, fa=None, fb=None):
    for k in INTS:
        assert np.array_equal(a[k], b[k]), k
    if fa is not None:
        assert fa.tobytes() == fb.tobytes()


def same_t(a, b):
    for k in ("t2d", "t1d_p1", "t1d_p2"):
        for x, y in zip(a[k], b[k]):
            assert gu.close(float(x), float(y)), (k, x, y)


def clean_rows(rg, ref, fst):
    """The rows post.region_scan is specified to build, from the oracle's records: one per region, the caller's
    order, an empty region with snp_count 0 and None everywhere."""
    slots, orec, ofst = ref
    by_slot, k = [], 0
    for (c, j, b, e) in slots:
        if b == e:
            row = dict.fromkeys(["snp_count", "T2D", "T1D_pop1", "T1D_pop2", "new_term_pop1", "new_term_pop2", "T2D_diff"])
            row["snp_count"] = 0
            if fst:
                row["FST"] = None
        else:
            o, f = orec[k], ofst[k]
            k += 1
            t2, t1, tb = o["T2D"], o["T1D_p1"], o["T1D_p2"]
            row = {"snp_count": o["snp_count"], "T2D": t2, "T1D_pop1": t1, "T1D_pop2": tb,
                   "new_term_pop1": None if t2 is None or t1 is None else t2 - t1,
                   "new_term_pop2": None if t2 is None or tb is None else t2 - tb,
                   "T2D_diff": None if None in (t2, t1, tb) else t2 - (t1 + tb) / 2}
            if fst:
                row["FST"] = f
        by_slot.append(row)
    return {key: by_slot[s] for key, s in zip(rg.keys(), rg.slot.tolist())}


def compare_rows(got, want):
    assert list(got) == list(want)
    got = {k: dict(r) for k, r in got.items()}
    for k in want:
        if "FST" in want[k]:
            g, f = got[k].pop("FST"), want[k]["FST"]
            assert (g is None) if f is None else abs(g - f) <= 1e-12 + 1e-10 * abs(f), (k, g, f)
    want = {k: {a: b for a, b in r.items() if a != "FST"} for k, r in want.items()}
    assert gu.compare_results(got, want) == []
