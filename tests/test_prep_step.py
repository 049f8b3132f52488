"""k_prep's step variants against the oracle: the joint-histogram step (a compile-time variant of k_prep,
2,048-SNP steps of 4 SNPs per lane) and the three-atomic step.  k_prep
writes only integers -- histograms, inner counts, slot bounds -- so what it determines is compared exactly
(Engine.bg_hist, the records' chrom / begin / end / snp_count / n2 / n1a / n1b); T values by
golden_util.close and Fst within 1e-12 + 1e-10 |x| of O.window_fst, as tests/test_scan_variants.py.

s is the step (2,048 SNPs); S = 2 s is the step of the 8-SNP-per-lane variant that was measured slower and
not kept -- the data sets keep its places, which are step, wave and lane edges of
the kept step too.  The benchmark's data set gets 65,536-SNP tiles from its size; these data sets are small,
so the tests ask for that tile (SFS2D_TILE), which also selects the joint histogram."""
import numpy as np
import pytest

import golden_util as gu
from oracle import sfs_oracle as O

pytestmark = pytest.mark.gpu

S, s = 4096, 2048
TILE = 65536
WS = 20000
_REF = {}


# ------------------------------------------------------------------------------------------- data sets

def _sprinkle(r1, a1, r2, a2, n1p, n2p, rng, every):
    """Key edge cases at random places (about one SNP in `every` each): the joint key 0 (a1 = a2 = 0), a
    folded SNP with the folded key 0 (r1 = r2 = 0), a1 + a2 exactly at the fold threshold and one above."""
    n = len(r1)
    n1, n2 = 2 * n1p, 2 * n2p
    kind = rng.integers(0, 4 * every, n)
    k = kind == 0
    r1[k], a1[k], r2[k], a2[k] = n1, 0, n2, 0
    k = kind == 1
    r1[k], a1[k], r2[k], a2[k] = 0, n1, 0, n2
    k = kind == 2
    r1[k], a1[k], r2[k], a2[k] = n1 - n1p, n1p, n2 - n2p, n2p
    k = kind == 3
    r1[k], a1[k], r2[k], a2[k] = n1 - n1p - 1, n1p + 1, n2 - n2p, n2p


def _with_counts(p, n1p, n2p, seed, overcall, every=40):
    from sfs2d.pack import PackedSNPs, pack_counts
    rng = np.random.default_rng(seed)
    r1, a1 = (p.counts & 0xff).astype(np.int64), ((p.counts >> 8) & 0xff).astype(np.int64)
    r2, a2 = ((p.counts >> 16) & 0xff).astype(np.int64), (p.counts >> 24).astype(np.int64)
    _sprinkle(r1, a1, r2, a2, n1p, n2p, rng, every)
    if overcall:   # r1 + 3 on unfolded SNPs, as test_prep_joint_histogram: the data set's nc_ok is false
        pick = (rng.random(p.n) < 0.0005) & (a1 + a2 <= n1p + n2p)
        assert pick.any()
        r1 = np.where(pick, r1 + 3, r1)
    return PackedSNPs(pack_counts(r1, a1, r2, a2), p.pos, p.chrom_off, p.chrom_names, p.ann_id, p.ann_names)


LENGTHS = [1, 7, 8, 9, s - 1, s + 1, S - 1, S, S + 1, 2 * S + 3, 65536 + S + 5]


def _lengths_genome(overcall):
    """Chromosomes of LENGTHS SNPs in that order (later ones start at offsets that are no multiple of 4 or
    8; the last spans two 65,536-SNP tiles), pop 25 / 25."""
    from sfs2d.synth import synth_genome
    p = synth_genome(len(LENGTHS), LENGTHS, 25, 25, seed=808)
    return _with_counts(p, 25, 25, 11, overcall)


def _positions(n, ws, starts, per_window):
    """Positions of n SNPs: a new window starts at every index in `starts` ({index: empty windows skipped
    before it}) and otherwise every `per_window` SNPs; SNPs of a window are 1 bp apart from its first bp."""
    pos = np.empty(n, np.int64)
    w, k = 0, 0
    for i in range(n):
        if i and (i in starts or k == per_window):
            w += 1 + starts.get(i, 0)
            k = 0
        pos[i] = w * ws + 1 + k
        k += 1
    assert per_window <= ws
    return pos


def _boundary_genome(overcall):
    """Two chromosomes of 65,536 + S + 5 SNPs with hand-placed 20 kb window boundaries, pop 25 / 25.  In
    the first (offset 0, so a lane's eight SNPs start at multiples of 8) a boundary falls between SNP 3 | 4
    of one lane's eight, between lanes 63 | 64, between the last SNP of a step and the first of the next and
    on the tile edge 65,535 | 65,536, each with adjacent windows; then the first three again across a gap of
    three empty windows.  The second chromosome starts at an offset that is 5 mod 8 and holds the same
    places relative to its own first tile, all across gaps, the tile edge included."""
    from sfs2d.pack import PackedSNPs
    from sfs2d.synth import synth_genome
    n = 65536 + S + 5
    p = synth_genome(2, [n, n], 25, 25, seed=4096)
    a = {2 * S + 8 * 10 + 4: 0, 3 * S + 8 * 64: 0, 5 * S: 0, 65536: 0,
         6 * S + 8 * 20 + 4: 3, 7 * S + 8 * 128: 3, 9 * S: 3}
    sh = n & 3   # the second chromosome's tiles start at the multiple of 4 below its first SNP
    b = {i - sh: 3 for i in a}
    pos = np.concatenate([_positions(n, WS, a, 3001), _positions(n, WS, b, 2777)]).astype(np.uint32)
    q = PackedSNPs(p.counts, pos, p.chrom_off, p.chrom_names, p.ann_id, p.ann_names)
    return _with_counts(q, 25, 25, 12, overcall)


def _small_grid_chrom(overcall):
    """One chromosome of 2 S SNPs, pop 3 / 2 (the 7-bin grid), 50 bp windows of 40 SNPs.  One lane's four
    SNPs [i0, i0 + 4) hold two boundaries, 0 | 1 and 2 | 3 (a two-SNP window opens and closes inside the lane,
    which writes slots of three windows); another lane's four hold a single-SNP window (boundaries 0 | 1 and
    1 | 2).  Both are inside one lane's eight as well."""
    from sfs2d.pack import PackedSNPs
    from sfs2d.synth import synth_genome
    n = 2 * S
    p = synth_genome(1, [n], 3, 2, seed=84)   # (the seed: see _cpu_check)
    i0 = S + 8 * 5
    j0 = i0 + 16
    pos = _positions(n, 50, {i0 + 1: 0, i0 + 3: 0, j0 + 1: 0, j0 + 2: 0}, 40).astype(np.uint32)
    q = PackedSNPs(p.counts, pos, p.chrom_off, p.chrom_names, p.ann_id, p.ann_names)
    return _with_counts(q, 3, 2, 13, overcall, every=25)


CASES = {"lengths": (_lengths_genome, 25, 25, WS), "boundaries": (_boundary_genome, 25, 25, WS),
         "small_grid": (_small_grid_chrom, 3, 2, 50)}


def _case(name, overcall):
    """(data, n1p, n2p, ws, (windows, oracle records, oracle Fst, backgrounds)), computed once and shared."""
    key = (name, overcall)
    if key not in _REF:
        make, n1p, n2p, ws = CASES[name]
        p = make(overcall)
        ocfg = O.Cfg(n1p, n2p)
        bgs = O.chrom_backgrounds(p, ocfg)
        wins = O.bp_windows(p, ws)
        recs = O.window_records(p, wins, ocfg, lambda c: bgs[c])
        fst = [O.window_fst(p, np.arange(w[2], w[3]), ocfg) for w in wins]
        _cpu_check(p, wins, recs)
        _REF[key] = (p, n1p, n2p, ws, (wins, recs, fst, bgs))
    return _REF[key]


def _cpu_check(p, wins, recs):
    """The fixture itself: every chromosome of >= 8 SNPs has a non-empty window, a T value is None only
    where its spectrum is empty, and no T value is a cancelled difference: a window's T is 2 sum x ln(x B /
    (N b)) over its bins, terms of up to N ln B <= 2e4 here (40 x ln 8192 = 360 on the 7-bin grid), so any
    evaluation order, the oracle's included, carries an absolute rounding error of ~1e-12 (1e-13), which
    1e-10 relative only covers for |T| >= 1e-2 (1e-3).  The generator seeds are fixed so that this holds."""
    small = p.n < 10000
    for o in recs:
        for t in ("T2D", "T1D_p1", "T1D_p2"):
            assert o[t] is None or o[t] == 0.0 or abs(o[t]) >= (1e-3 if small else 1e-2), (t, o[t])
    have = {w[0] for w in wins}
    for c in range(p.nchrom):
        if p.chrom_off[c + 1] - p.chrom_off[c] >= 8:
            assert c in have, c
    for o in recs:
        for t, cnt in (("T2D", "N2"), ("T1D_p1", "N1a"), ("T1D_p2", "N1b")):
            assert o[t] is not None or o[cnt] == 0, (t, o)


# --------------------------------------------------------------------------------------------- checks

def _run(p, n1p, n2p, ws, runs=1):
    """`runs` runs of one plan (Fst on): [(records, Fst), ...]."""
    from sfs2d.engine import Engine, ScanConfig
    eng = Engine.get(0)
    dev = eng.upload(p)
    pl = eng.plan(dev, ScanConfig(n1p=n1p, n2p=n2p, window=ws, fst=True))
    out = []
    for _ in range(runs):
        pl.run()
        pl.check()
        out.append((pl.read(), pl.read_fst()))
    pl.close()
    dev.close()
    return out


def _check(recs, fst, ref):
    from sfs2d import _lib as L
    wins, orec, ofst, _ = ref
    live = (recs["flags"] & L.W_EMPTY) == 0
    body = recs[live]
    assert len(body) == len(wins), (len(body), len(wins))
    fl = fst[: len(live)][live[: len(fst)]]
    assert len(fl) == len(wins)
    for i, (w, r, o, f) in enumerate(zip(wins, body, orec, ofst)):
        assert (int(r["chrom"]), int(r["begin"]), int(r["end"])) == (w[0], w[2], w[3]), (i, w)
        for a, b in (("snp_count", "snp_count"), ("n2", "N2"), ("n1a", "N1a"), ("n1b", "N1b")):
            assert int(r[a]) == o[b], (i, a, int(r[a]), o[b])
        for a, b in (("t2d", "T2D"), ("t1d_p1", "T1D_p1"), ("t1d_p2", "T1D_p2")):
            if o[b] is not None:
                assert gu.close(float(r[a]), o[b]), (i, a, float(r[a]), o[b])
        g = float(fl[i])
        assert (np.isnan(g) if f is None else abs(g - f) <= 1e-12 + 1e-10 * abs(f)), (i, "fst", g, f)


def _check_bg_hist(p, n1p, n2p, bgs, chroms):
    import twoDSFS_class as T
    from sfs2d.engine import Engine, ScanConfig
    eng = Engine.get(0)
    dev = eng.upload(p)
    for c in chroms:
        h2, u1, u2 = eng.bg_hist(dev, ScanConfig(n1p=n1p, n2p=n2p), c)
        assert np.array_equal(np.asarray(h2), np.asarray(bgs[c][0])), c
        assert np.array_equal(T._fold_counts(u1), np.asarray(bgs[c][1])), c
        assert np.array_equal(T._fold_counts(u2), np.asarray(bgs[c][2])), c
    dev.close()


# ---------------------------------------------------------------------------------------------- tests

@pytest.mark.parametrize("overcall", [False, True])
@pytest.mark.parametrize("name", ["lengths", "boundaries", "small_grid"])
def test_joint_step_vs_oracle(monkeypatch, name, overcall):
    """The joint-histogram step (65,536-SNP tiles) against the oracle, window by window, with and
    without over-called SNPs (without: nc_ok, no step takes the exact path for its counts); every chromosome's
    background histograms exactly."""
    monkeypatch.setenv("SFS2D_TILE", str(TILE))
    monkeypatch.delenv("SFS2D_JNT", raising=False)
    p, n1p, n2p, ws, ref = _case(name, overcall)
    (recs, fst), = _run(p, n1p, n2p, ws)
    _check(recs, fst, ref)
    _check_bg_hist(p, n1p, n2p, ref[3], range(p.nchrom))


@pytest.mark.parametrize("name", ["boundaries", "small_grid"])
def test_small_tiles_vs_oracle(monkeypatch, name):
    """The same places with 4,096-SNP tiles (two steps each: every tile edge is a step edge)."""
    monkeypatch.setenv("SFS2D_TILE", str(S))
    monkeypatch.setenv("SFS2D_JNT", "1")
    p, n1p, n2p, ws, ref = _case(name, True)
    (recs, fst), = _run(p, n1p, n2p, ws)
    _check(recs, fst, ref)


@pytest.mark.parametrize("overcall", [False, True])
def test_variants_agree(monkeypatch, overcall):
    """Records and Fst of the lengths genome byte-equal across the joint histogram and the three atomics, and
    across tile sizes (65,536, 8,192, 4,096, 2,048 and the size's own default); a second run of the same plan byte-equal to the first (replica parity, cleared LDS / slot state)."""
    p, n1p, n2p, ws, ref = _case("lengths", overcall)
    out = {}
    for jnt, tile in (("1", TILE), ("0", TILE), ("1", 8192), ("1", S), ("1", s), ("0", s), (None, None)):
        for k, v in (("SFS2D_JNT", jnt), ("SFS2D_TILE", tile)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
        runs = _run(p, n1p, n2p, ws, runs=2 if tile in (TILE, s) else 1)
        for r, f in runs[1:]:
            assert r.tobytes() == runs[0][0].tobytes() and f.tobytes() == runs[0][1].tobytes(), (jnt, tile)
        out[(jnt, tile)] = runs[0]
    first = out[("1", TILE)]
    _check(first[0], first[1], ref)
    for key, (r, f) in out.items():
        assert r.tobytes() == first[0].tobytes(), key
        assert f.tobytes() == first[1].tobytes(), key
