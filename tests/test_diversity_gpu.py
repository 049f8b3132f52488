"""Per-window diversity on the device (kernel k_div_win, sfs2d_plan_diversity) against the
numpy definition of tests/div_util.py, window by window: integer fields exact, doubles within the project's 1e-10
relative (golden_util.close), an expected 0.0 exactly 0.0.

The genome has ~1e4 SNPs in chromosomes of 6,000 / 1 / 3,584 SNPs (a chromosome of one SNP; 3,584 = 7 x 512, so
SNP-count windows of 1, 64 and 512 end on the data set's last SNP), pop (18, 14).  Awkward SNPs sit at the row
edges of the kernel's load loop (a row is 64 SNPs, a block eight rows): n = 0 or 1 called alleles in one population
and in both, sites fixed for the reference or the alternative allele with missing calls, over-called SNPs
(n > 2 pop_size), between fully called ones.  A window's sums have at most a few hundred terms of one sign, each
<= 1, summed per lane and then over the wave: the relative error is a few hundred eps, far inside 1e-10."""
import csv
import ctypes as C
import os

import numpy as np
import pytest

import div_util as DU
from golden_util import GOLD, close
from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import diversity as DV

pytestmark = pytest.mark.gpu

N1P, N2P = 18, 14
LENGTHS = [6000, 1, 3584]
VT = "intron_variant"
_DATA = {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE", "SFS2D_SLOTS_ONCE"):
        monkeypatch.delenv(k, raising=False)


def _awkward(n1, n2):
    """SNPs whose terms are easy to get wrong, all with alt counts <= 2 pop_size and keys inside the grid."""
    return [(0, 0, n2 - 8, 8), (n1 - 5, 5, 0, 0), (1, 0, n2 - 3, 3), (0, 1, 5, n2 - 5), (n1 - 9, 9, 1, 0), (4, n1 - 4, 0, 1),
            (0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 1, 0), (1, 0, 0, 0),                        # n <= 1 in both
            (n1 - 2, 0, n2 - 1, 0), (n1, 0, n2 - 6, 0), (0, n1 - 3, 0, n2), (0, n1, 0, n2 - 2),   # fixed, missing calls
            (n1 - 4, 0, 0, n2 - 1), (0, n1 - 1, n2 - 2, 0),                               # fixed differently: dxy = 1
            (n1 - 7, 7, n2 - 9, 9), (n1 - 1, 1, n2 - 1, 1), (3, n1 - 3, 2, n2 - 2),         # fully called
            (n1 - 9, 6, n2 - 4, 3), (5, 6, 7, 4)]                                          # missing calls, segregating


def _genome(n1p=N1P, n2p=N2P, overcall=False):
    key = (n1p, n2p, overcall)
    if key in _DATA:
        return _DATA[key]
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_genome
    p = synth_genome(3, LENGTHS, n1p, n2p, seed=29 + n1p, n_ann=3)
    n1, n2 = 2 * n1p, 2 * n2p
    r = [p.ref1.copy(), p.alt1.copy(), p.ref2.copy(), p.alt2.copy()]
    aw = _awkward(n1, n2)
    # at the row edges (63 | 64), the block edges (511 | 512), the data set's ends, and one dense run of them
    at = [0, 1, 62, 63, 64, 65, 127, 128, 510, 511, 512, 513, 1023, 1024, 5999, 6000, 6001, 6002, 9583, 9584]
    at += list(range(2040, 2040 + 2 * len(aw)))
    for k, i in enumerate(at):
        for f, v in zip(r, aw[k % len(aw)]):
            f[i] = v
    if overcall:   # called counts above 2 pop_size, alt counts within it, the folded key inside the grid
        rng = np.random.default_rng(5)
        for i in rng.choice(p.n, 300, replace=False).tolist() + [66, 514, 2100]:
            r[0][i], r[1][i] = rng.integers(n1p + 1, n1 + 1), rng.integers(n1p, int(n1 * 0.7) + 1)
            r[2][i], r[3][i] = rng.integers(n2p - 4, n2 + 1), rng.integers(n2p + 1, int(n2 * 0.7) + 1)
        assert np.any(r[0] + r[1] > n1) and np.any(r[2] + r[3] > n2)
    q = PackedSNPs(pack_counts(*r), p.pos, p.chrom_off, p.chrom_names, p.ann_id, p.ann_names)
    _DATA[key] = q
    return q


def _engine():
    from sfs2d.engine import Engine
    return Engine.get(0)


def _cfg(**kw):
    from sfs2d.engine import ScanConfig
    kw.setdefault("n1p", N1P)
    kw.setdefault("n2p", N2P)
    return ScanConfig(**kw)


def _ocfg(cfg, p):
    vt = None if cfg.ann_want < 0 else p.ann_names[cfg.ann_want]
    return O.Cfg(cfg.n1p, cfg.n2p, vt, cfg.fold, cfg.start_position, cfg.end_position)


class _Run:
    """A plan over an uploaded genome, run once; closes both."""

    def __init__(self, p, cfg, bg=None, run=True):
        self.p, self.cfg = p, cfg
        self.dev = _engine().upload(p)
        try:
            self.pl = _engine().plan(self.dev, cfg)
            if bg is not None:
                self.pl.set_background(*bg)
            if run:
                self.pl.run()
                self.pl.check()
        except Exception:
            self.dev.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.pl.close()
        self.dev.close()


def _check_plan(p, pl, cfg, what=""):
    """The plan's diversity records against the helper's over the plan's own record ranges; returns (recs, div)."""
    recs, div = pl.read(), pl.diversity()
    assert len(div) == len(recs) == pl.nrec
    DU.assert_records(div, DU.expected_for_records(p, recs, _ocfg(cfg, p)), what)
    return recs, div


# ------------------------------------------------------------------------------------------- window sizes

@pytest.mark.parametrize("S", [1, 63, 64, 65, 511, 512, 513])
def test_snp_count_windows(S):
    """The row edge (64) and the eight-row block edge (512) of the load loop, one SNP either side."""
    p = _genome()
    cfg = _cfg(window_mode=L.WINDOW_SNPS, window=S)
    with _Run(p, cfg) as r:
        recs, div = _check_plan(p, r.pl, cfg, f"S={S}")
    wins, _ = O.snp_windows(p, S)
    assert [(int(b), int(e)) for b, e in zip(recs["begin"], recs["end"])] == [(w[3], w[4]) for w in wins]
    assert (int(recs["end"].max()) == p.n) == (S in (1, 64, 512))          # a window ending on the last SNP
    assert (recs["chrom"] == 1).sum() == (1 if S == 1 else 0)               # the one-SNP chromosome
    assert div["s1"].sum() > 0 and div["s1_full"].sum() > 0 and (div["s1"] != div["s1_full"]).any()
    if S == 1:   # single SNPs: the awkward ones give exact zeros
        assert _awkward(36, 28)[7] == (1, 0, 0, 1)          # placed at SNP 128 (the eighth of _genome's places)
        assert float(div["dxy"][128]) == 1.0 and float(div["pi1"][128]) == 0.0 and div["s1"][128] == 0


FILTERS = {"counts": {}, "pos": {"start_position": 40000, "end_position": 250000}, "vt": {"ann_want": 1},
           "both": {"start_position": 40000, "end_position": 250000, "ann_want": 1}}


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
@pytest.mark.parametrize("filt", list(FILTERS))
def test_fixed_bp_counts_and_filtered_plans(filt, fold):
    """Fixed-bp windows with empty slots between SNPs; counts plans and the three kinds of filtered plans."""
    p = _genome()
    assert p.ann_names[1] == VT
    cfg = _cfg(window=200, fold=fold, fst=True, **FILTERS[filt])
    with _Run(p, cfg) as r:
        assert r.pl.scan_variant()["cnt"] == (1 if filt == "counts" else 0)
        recs, div = _check_plan(p, r.pl, cfg, filt)
    empty = (recs["flags"] & L.W_EMPTY) != 0
    assert empty.any() and (div["flags"][empty] == L.W_EMPTY).all() and (div["flags"][~empty] == 0).all()
    assert int(recs["end"][~empty].max()) == p.n
    one = recs[(recs["chrom"] == 1) & ~empty]
    assert len(one) == 1 and one["end"][0] - one["begin"][0] == 1
    if filt != "counts":   # the filters take SNPs out of the sums
        allin = DU.expected_for_records(p, recs, O.Cfg(N1P, N2P, None, fold))
        assert (div["s1"] < allin["s1"]).any() and (div["s1"] <= allin["s1"]).all()
    # wider windows, of several rows each
    cfg = _cfg(window=30000, fold=fold, **FILTERS[filt])
    with _Run(p, cfg) as r:
        recs, _ = _check_plan(p, r.pl, cfg, filt + " 30kb")
    assert (recs["end"] - recs["begin"]).max() > 128


def test_overcalled_snps():
    """SNPs with more called alleles than 2 pop_size: in pi, S and theta with their own n, never fully called."""
    p = _genome(overcall=True)
    for mode, w in ((L.WINDOW_BP, 20000), (L.WINDOW_SNPS, 65)):
        cfg = _cfg(window_mode=mode, window=w)
        with _Run(p, cfg) as r:
            recs, div = _check_plan(p, r.pl, cfg, f"overcalled {w}")
        assert (div["s1"] > div["s1_full"]).any()


def test_large_grid_plan():
    """pop 50 / 50: k_scan_gw's records are read like the others."""
    p = _genome(50, 50)
    cfg = _cfg(n1p=50, n2p=50, window=15000)
    with _Run(p, cfg) as r:
        assert r.pl.scan_kernel() == "k_scan_gw"
        _, div = _check_plan(p, r.pl, cfg, "gw")
    assert div["s2_full"].sum() > 0
    cfg = _cfg(n1p=50, n2p=50, window_mode=L.WINDOW_SNPS, window=513, ann_want=2, fold=False)
    with _Run(p, cfg) as r:
        _check_plan(p, r.pl, cfg, "gw filtered")


def _slide_ranges(p, W, step):
    out = []
    for c in range(p.nchrom):
        s, e = int(p.chrom_off[c]), int(p.chrom_off[c + 1])
        pos = p.pos[s:e].astype(np.int64)
        for j in range((int(pos[-1]) - 1) // step + 1):
            out.append((s + int(np.searchsorted(pos, j * step + 1, "left")), s + int(np.searchsorted(pos, j * step + W, "right"))))
    return out


def test_sliding_plan():
    p = _genome()
    W, step = 8000, 2000   # m = 4
    cfg = _cfg(window=W, step=step, fst=True)
    with _Run(p, cfg) as r:
        recs, div = _check_plan(p, r.pl, cfg, "sliding")
    rng = _slide_ranges(p, W, step)
    live = (recs["flags"] & L.W_EMPTY) == 0
    assert len(rng) == len(recs)
    assert [(int(b), int(e)) for b, e in zip(recs["begin"][live], recs["end"][live])] == [x for x, k in zip(rng, live) if k]
    assert all(b == e for (b, e), k in zip(rng, live) if not k)


@pytest.mark.parametrize("base_step", [None, 1000], ids=["ordinary_base", "sliding_base"])
def test_attached_plans(base_step):
    """Attached plans have their own records and share the base's data (and, filtered, its per-SNP bins)."""
    p = _genome()
    for filt in ({}, {"ann_want": 1, "start_position": 40000}):
        base_cfg = _cfg(window=2000, step=base_step, **filt)
        with _Run(p, base_cfg, run=False) as r:
            if base_step is None:
                cfgs = [_cfg(window=10000, **filt), _cfg(window_mode=L.WINDOW_SNPS, window=65, **filt)]
            else:
                cfgs = [_cfg(window=4000, step=base_step, **filt)]
            att = [r.pl.attach(c) for c in cfgs]
            with pytest.raises(L.Sfs2dError) as ei:      # an attached plan has no records before its base runs
                att[0].diversity()
            assert ei.value.code == L.E_ARG
            r.pl.run()
            r.pl.check()
            brecs, _ = _check_plan(p, r.pl, base_cfg, "base")
            for a, c in zip(att, cfgs):
                recs, _ = _check_plan(p, a, c, f"attached {c.window}")
                assert recs[["begin", "end"]].tobytes() != brecs[["begin", "end"]].tobytes()     # windows of its own


def test_prev_extra_record_is_flagged_and_zero():
    p = _genome()
    cfg = _cfg(window=20000, prev_extra=True)
    with _Run(p, cfg) as r:
        recs, div = _check_plan(p, r.pl, cfg, "prev_extra")
    assert recs[-1]["flags"] & L.W_EXTRA and recs[-1]["end"] > recs[-1]["begin"]      # it has a range of its own
    assert div[-1]["flags"] == L.W_EXTRA
    z = np.zeros(1, L.DIVERSITY_DTYPE)
    z["flags"] = L.W_EXTRA
    assert div[-1:].tobytes() == z.tobytes()


# ------------------------------------------------------------------------------------------- determinism

def test_two_calls_are_byte_equal():
    p = _genome()
    for cfg in (_cfg(window=20000), _cfg(window_mode=L.WINDOW_SNPS, window=513, ann_want=1)):
        with _Run(p, cfg) as r:
            a = r.pl.diversity()
            b = r.pl.diversity()
            assert a.tobytes() == b.tobytes() and a["s1"].sum() > 0


@pytest.mark.parametrize("null", [False, True], ids=["div", "div_null_div"])
@pytest.mark.parametrize("fused", ["0", "1"], ids=["sliced", "fused"])
def test_following_runs_are_untouched(monkeypatch, fused, null):
    """run, diversity, run (and once more: both replica parities) leaves the later runs' records and Fst
    byte-equal to a plan that never called it; the same with a null run between two diversity calls."""
    monkeypatch.setenv("SFS2D_FUSED", fused)
    p = _genome()
    cfg = _cfg(window=5000, fst=True, prev_extra=True)
    with _Run(p, cfg) as ref:
        assert ref.pl.scan_variant()["fused"] == int(fused)
        want = []
        for _ in range(2):
            ref.pl.run()
            ref.pl.check()
            want.append((ref.pl.read().tobytes(), ref.pl.read_fst().tobytes()))
    with _Run(p, cfg) as r:
        first = None
        for k in range(2):
            d = r.pl.diversity()
            if null:
                r.pl.null_run([(0, 65), (2, 513)], 8, 3)
                assert r.pl.diversity().tobytes() == d.tobytes()
            first = d if first is None else first
            assert d.tobytes() == first.tobytes()          # the same data, the same windows: every run alike
            r.pl.run()
            r.pl.check()
            assert (r.pl.read().tobytes(), r.pl.read_fst().tobytes()) == want[k], k
        _check_plan(p, r.pl, cfg, "after")


# ------------------------------------------------------------------------------------------- refusals

def test_refusals():
    p = _genome()
    cfg = _cfg(window=20000)
    with _Run(p, cfg, run=False) as r:
        with pytest.raises(L.Sfs2dError) as ei:
            r.pl.diversity()
        assert ei.value.code == L.E_ARG and "first run" in str(ei.value)
        lib = r.pl.eng.lib
        n = C.c_int64()
        buf = np.zeros(r.pl.nrec, L.DIVERSITY_DTYPE)
        assert lib.sfs2d_plan_diversity_read(r.pl.h, L.ptr(buf), r.pl.nrec, C.byref(n)) == L.E_ARG     # no call yet
        r.pl.run()
        r.pl.check()
        assert lib.sfs2d_plan_diversity(r.pl.h, None) == 0
        assert lib.sfs2d_plan_diversity_read(r.pl.h, L.ptr(buf), r.pl.nrec - 1, C.byref(n)) == L.E_CAP
        assert n.value == r.pl.nrec
        assert lib.sfs2d_plan_diversity_read(r.pl.h, L.ptr(buf), r.pl.nrec, C.byref(n)) == 0
        assert buf.tobytes() == r.pl.diversity().tobytes()


def test_caller_buffer():
    import torch
    p = _genome()
    cfg = _cfg(window=20000)
    with _Run(p, cfg) as r:
        want = r.pl.diversity()
        buf = torch.zeros(r.pl.nrec * L.DIVERSITY_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert r.pl.diversity(out_dev_ptr=buf.data_ptr()) is None
        r.pl.check()                                           # synchronises the engine's stream
        got = np.frombuffer(buf.cpu().numpy().tobytes(), L.DIVERSITY_DTYPE)
        assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------- class and CLI

def _expected_rows(p, kind, w, ocfg):
    """{label: the twelve columns} from the oracle's windows and the helper's sums."""
    names = p.chrom_names
    if kind == "bp":
        wins = [(f"{names[c]} {s}-{s + w - 1}", b, e, float(w)) for c, s, b, e in O.bp_windows(p, w)]
    else:
        wins = [(f"{names[c]} {sp}-{ep}", b, e, float(int(p.pos[e - 1]) - int(p.pos[b]) + 1))
                for c, sp, ep, b, e in O.snp_windows(p, w)[0]]
    d = DU.expected(p, [(b, e) for _, b, e, _ in wins], ocfg)
    out = {}
    for (lb, _, _, span), x in zip(wins, d):
        pi1, pi2, dxy = float(x["pi1"]) / span, float(x["pi2"]) / span, float(x["dxy"]) / span
        out[lb] = {"pi_pop1": pi1, "pi_pop2": pi2, "dxy": dxy, "da": dxy - (pi1 + pi2) / 2,
                   "theta_w_pop1": float(x["thw1"]) / span, "theta_w_pop2": float(x["thw2"]) / span,
                   "S_pop1": int(x["s1"]), "S_pop2": int(x["s2"]), "S_full_pop1": int(x["s1_full"]),
                   "S_full_pop2": int(x["s2_full"]),
                   "tajima_d_pop1": DV.tajima_d(2 * ocfg.n1p, x["s1_full"], x["ar1_full"]),
                   "tajima_d_pop2": DV.tajima_d(2 * ocfg.n2p, x["s2_full"], x["ar2_full"])}
    return out


def _rows_close(got, want, what):
    assert list(got) == DV.KEYS, (what, list(got))
    for k in DV.KEYS:
        if k.startswith("S_"):
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:   # da is a difference: relative to its operands
            assert close(got[k], want[k], scale=want["dxy"] if k == "da" else None), (what, k, got[k], want[k])


def test_class_window_diversity_and_multi_scan():
    import twoDSFS_class as T
    p = _genome()
    ocfg = O.Cfg(N1P, N2P)
    obj = T.LikelihoodInference_jointSFS(None, None, pop1_size=N1P, pop2_size=N2P)
    for kw, kind, w in (({"window_size": 20000}, "bp", 20000), ({"snp_window_size": 300}, "snps", 300)):
        got, want = obj.window_diversity(p, **kw), _expected_rows(p, kind, w, ocfg)
        assert list(got) == list(want) and len(got) > 5
        for lb in want:
            _rows_close(got[lb], want[lb], lb)
    assert any(r["tajima_d_pop1"] is not None for r in got.values())
    sl = obj.window_diversity(p, window_size=8000, step_size=2000)
    assert list(sl) == list(obj.sliding_scan(p, 8000, 2000))
    res = obj.multi_scan(p, [20000, 60000], [300], fst=True, diversity=True)
    plain = obj.multi_scan(p, [20000, 60000], [300], fst=True)
    for key, kind, w in ((20000, "bp", 20000), (60000, "bp", 60000), ("300snps", "snps", 300)):
        want = _expected_rows(p, kind, w, ocfg)
        assert list(res[key]) == list(plain[key]) and len(res[key]) > 2
        for lb, row in res[key].items():
            assert {k: v for k, v in row.items() if k not in DV.KEYS} == plain[key][lb]
            _rows_close({k: row[k] for k in DV.KEYS}, want[lb], lb)
    assert res["fst"] == plain["fst"]
    pv = obj.scan_pvalues(p, [20000], replicates=19, seed=1, diversity=True)
    for lb, row in pv[20000].items():
        _rows_close({k: row[k] for k in DV.KEYS}, _expected_rows(p, "bp", 20000, ocfg)[lb], lb)
        assert "p_T2D" in row


def test_cli_diversity_columns(tmp_path):
    import twoDSFS_class as T
    from sfs2d import cli
    from sfs2d.vcf import read_vcf
    vcf, pm = os.path.join(GOLD, "vcf_test.vcf.gz"), os.path.join(GOLD, "popmap_3pop.txt")
    p = read_vcf(vcf, pm).to_packed("uv", "bv")
    ocfg = O.Cfg(11, 11)
    base = [vcf, pm, "--pop1", "uv", "--pop2", "bv", "--pop1-size", "11", "--pop2-size", "11", "--fst",
            "--window", "500000", "--snp-window", "100"]
    outs = cli.main(base + ["--diversity", "--out-prefix", str(tmp_path / "d")])
    plain = cli.main(base + ["--out-prefix", str(tmp_path / "p")])
    for path, ppath, kind, w in ((outs[0], plain[0], "bp", 500000), (outs[1], plain[1], "snps", 100)):
        with open(path, newline="") as fh:
            rows = list(csv.DictReader(fh))
        with open(ppath, newline="") as fh:
            prow = list(csv.DictReader(fh))
        assert list(rows[0]) == T.col_names + ["FST"] + DV.KEYS and list(prow[0]) == T.col_names + ["FST"]
        assert [{k: r[k] for k in prow[0]} for r in rows] == prow
        want = _expected_rows(p, kind, w, ocfg)
        assert len(rows) > 3
        for r in rows:
            x = want[f"{r['chromosome']} {r['window_start']}-{r['window_end']}"]
            got = {k: (None if r[k] == "" else int(r[k]) if k.startswith("S_") else float(r[k])) for k in DV.KEYS}
            _rows_close(got, x, r["window_start"])
