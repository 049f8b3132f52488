"""Test-only: the small genome and the oracle reference of the window-spectra tests (test_spectra_gpu.py).

The genome (``genome``): chromosomes of 1, 63, 64, 65, 255, 256, 257, 2,047, 2,049 and 9,000 SNPs, so that whole-
chromosome records sit on, one below and one above a wavefront row (64 SNPs), a workgroup row (256) and the
kernel's block of rows in flight (8 x 256 = 2,048).  Planted among the generated SNPs, at the row edges and every
41st SNP, are the kinds a wrong shortcut would miscount (``PLANTED``); ``assert_kinds`` asserts on the oracle's
output that the fixture holds every one of them.

``expected`` builds the rows sfs2d_plan_spectra is specified to give from oracle.sfs2d / sfs1d / fold1d of each
record's own range: [grid | fold1d(sfs1d pop 1) with entries 0 and n1p zeroed | the same for pop 2], summed per
group.  An oracle row is computed once per (data, range, configuration) and shared."""
import numpy as np

from oracle import sfs_oracle as O
from sfs2d import _lib as L

LENGTHS = [1, 63, 64, 65, 255, 256, 257, 2047, 2049, 9000]
VT = "intron_variant"
_DATA, _ROWS = {}, {}


def planted(n1p, n2p):
    """(ref1, alt1, ref2, alt2) by kind; every alt count <= 2 pop_size and every folded key inside the grid."""
    n1, n2 = 2 * n1p, 2 * n2p
    return {
        "last_bin_unfolded": (0, n1, 0, n2),                     # (n1, n2) without the fold; folded: (0, 0), 1D bin 0
        "last_bin_folded": (n1, n1p + 1, n2, n2p),               # over-called; the fold swaps to the refs (n1, n2)
        "zero_zero": (n1 - 1, 0, n2, 0),                         # fixed for the reference allele in both
        "folded": (3, n1 - 3, 2, n2 - 2),                        # alt1 + alt2 > n1p + n2p: key (3, 2)
        "fold_tie": (n1 - n1p - 3, n1p + 3, n2 - n2p + 3, n2p - 3),   # alt1 + alt2 == n1p + n2p: not folded
        "over_called": (n1 - 2, 5, n2 - 1, 2),                   # r + a > 2 pop_size, key (5, 2) inside the grid
        "fold1d_bin_np": (n1p, n1p, n2p - 1, n2p),               # folded 1D bin n_p in both populations
        "fold1d_bin_0": (0, n1, 4, n2 - 4 - 1),                  # alt1 == n1: folded 1D bin 0 of population 1
    }


def genome(n1p, n2p, lengths=None, seed=None, plant=True):
    """``plant`` False (the large grids, whose over-called last-bin SNP would not fit the u8 counts): the generated
    SNPs alone."""
    lengths = LENGTHS if lengths is None else list(lengths)
    key = (n1p, n2p, tuple(lengths), plant)
    if key in _DATA:
        return _DATA[key]
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_genome
    p = synth_genome(len(lengths), lengths, n1p, n2p, seed=(seed or 170) + n1p, n_ann=3)
    r = [p.ref1.copy(), p.alt1.copy(), p.ref2.copy(), p.alt2.copy()]
    kinds = list(planted(n1p, n2p).values())
    big = int(p.chrom_off[-2])   # the last chromosome's first SNP
    at = sorted(set(list(range(5, p.n, 41)) + [big + x for x in (0, 63, 64, 255, 256, 257, 2047, 2048, 2049)
                                               if big + x < p.n] + [p.n - 1]))
    for k, i in enumerate(at if plant else []):
        for f, v in zip(r, kinds[k % len(kinds)]):
            f[i] = v
    q = PackedSNPs(pack_counts(*r), p.pos, p.chrom_off, p.chrom_names, p.ann_id, p.ann_names)
    _DATA[key] = q
    return q


def assert_kinds(p, n1p, n2p):
    """The fixture's properties, on the oracle's output."""
    fold, nofold = O.Cfg(n1p, n2p, None, True), O.Cfg(n1p, n2p, None, False)
    allidx = np.arange(p.n)
    gf, gn = O.sfs2d(p, allidx, fold), O.sfs2d(p, allidx, nofold)
    assert p.n - gf.sum() > 0 and p.n - gn.sum() > 0                 # (0, 0) SNPs: skipped
    assert gf[-1, -1] > 0 and gn[-1, -1] > 0                         # last-bin SNPs, with and without the fold
    assert (gf != gn).any()                                          # folded SNPs
    kinds = planted(n1p, n2p)
    r1, a1, r2, a2 = (x.astype(np.int64) for x in (p.ref1, p.alt1, p.ref2, p.alt2))

    def where(kind):
        v = kinds[kind]
        i = np.nonzero((r1 == v[0]) & (a1 == v[1]) & (r2 == v[2]) & (a2 == v[3]))[0]
        assert i.size, kind
        return int(i[0])
    i = where("fold_tie")
    assert a1[i] + a2[i] == n1p + n2p and (r1[i], r2[i]) != (a1[i], a2[i])
    assert np.array_equal(O.sfs2d(p, [i], fold), O.sfs2d(p, [i], nofold))            # the tie is not folded
    i = where("over_called")
    assert r1[i] + a1[i] > 2 * n1p and r2[i] + a2[i] > 2 * n2p
    assert O.sfs2d(p, [i], fold).sum() == 1 and O.sfs2d(p, [i], fold)[5, 2] == 1    # counted, inside the grid
    i = where("last_bin_folded")
    assert O.sfs2d(p, [i], fold)[-1, -1] == 1
    f1 = O.fold1d(O.sfs1d(p, allidx, 1, fold))
    f2 = O.fold1d(O.sfs1d(p, allidx, 2, fold))
    assert f1[0] > 0 and f1[n1p] > 0 and f2[n2p] > 0                 # folded 1D bins 0 and n_p: not exported


def ocfg_of(cfg, p):
    vt = None if cfg.ann_want < 0 else p.ann_names[cfg.ann_want]
    return O.Cfg(cfg.n1p, cfg.n2p, vt, cfg.fold, cfg.start_position, cfg.end_position)


def oracle_row(p, b, e, ocfg):
    """One record's row from the oracle (cached; treat as read-only)."""
    key = (id(p), int(b), int(e), ocfg.n1p, ocfg.n2p, ocfg.variant_type, ocfg.fold, ocfg.start_position, ocfg.end_position)
    row = _ROWS.get(key)
    if row is None:
        idx = np.arange(int(b), int(e))
        f1 = O.fold1d(O.sfs1d(p, idx, 1, ocfg))
        f2 = O.fold1d(O.sfs1d(p, idx, 2, ocfg))
        e1, e2 = np.zeros(ocfg.n1p + 1, np.int64), np.zeros(ocfg.n2p + 1, np.int64)
        e1[1:ocfg.n1p] = f1[1:ocfg.n1p]
        e2[1:ocfg.n2p] = f2[1:ocfg.n2p]
        row = np.concatenate([O.sfs2d(p, idx, ocfg).ravel(), e1, e2]).astype(np.int64)
        assert row.size == L.spec_row_words(ocfg.n1p, ocfg.n2p)
        row.setflags(write=False)
        _ROWS[key] = row
    return row


def expected(p, recs, ocfg, rec=None, grp=None, ngroups=None):
    """int64[ngroups, row words]: per group the sum over its entries of the oracle's row of the record's own range
    (clamped to the data set); EMPTY and EXTRA records add nothing."""
    rec = np.arange(len(recs)) if rec is None else np.asarray(rec, np.int64)
    grp = np.arange(len(rec)) if grp is None else np.asarray(grp, np.int64)
    if ngroups is None:
        ngroups = max(1, int(grp.max()) + 1 if len(grp) else 1)
    out = np.zeros((ngroups, L.spec_row_words(ocfg.n1p, ocfg.n2p)), np.int64)
    for s, g in zip(rec.tolist(), grp.tolist()):
        r = recs[s]
        if int(r["flags"]) & (L.W_EMPTY | L.W_EXTRA):
            continue
        e = min(int(r["end"]), p.n)
        out[g] += oracle_row(p, min(int(r["begin"]), e), e, ocfg)
    return out


def assert_rows(got, want, what=""):
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        g, k = np.nonzero(got != want)
        raise AssertionError((what, "first differing (group, word)", int(g[0]), int(k[0]), int(got[g[0], k[0]]),
                              int(want[g[0], k[0]]), "groups differing", int(np.unique(g).size)))


class Run:
    """A plan over an uploaded (or given) data set, run once; closes what it opened."""

    def __init__(self, p, cfg, bg=None, run=True, dev=None):
        from sfs2d.engine import Engine
        eng = Engine.get(0)
        self.p, self.cfg, self.own = p, cfg, dev is None
        self.dev = eng.upload(p) if dev is None else dev
        try:
            self.pl = eng.plan(self.dev, cfg)
            if bg is not None:
                self.pl.set_background(*bg)
            if run:
                self.pl.run()
                self.pl.check()
        except Exception:
            if self.own:
                self.dev.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.pl.close()
        if self.own:
            self.dev.close()
