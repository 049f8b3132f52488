"""Per-window diversity without a GPU: the definitions on hand-computed SNPs, Tajima's D,
the host twin against the test helper, the per-site rows on fake records, the CSV columns and the record layout.

The hand-computed terms use tests/div_util.py's per-SNP definition (plain Python numbers) and
sfs2d.diversity.window_sums side by side; neither is used to make the expected values."""
import csv
import os
import re

import numpy as np
import pytest

import div_util as DU
import fake_records as FR
from golden_util import close
from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import cli, post
from sfs2d import diversity as DV
from sfs2d.pack import PackedSNPs, pack_counts

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _packed(snps, pos=None, n_ann=None):
    a = np.array(snps, np.int64).reshape(-1, 4)
    pos = np.arange(1, len(a) + 1) * 10 if pos is None else pos
    return PackedSNPs(pack_counts(a[:, 0], a[:, 1], a[:, 2], a[:, 3]), np.asarray(pos, np.uint32),
                      np.array([0, len(a)], np.int64), ["c1"], np.zeros(len(a), np.uint16), ["x"])


def _sums(snps, n1p=2, n2p=2, fold=False):
    p = _packed(snps)
    return DV.window_sums(p, 0, p.n, O.Cfg(n1p, n2p, None, fold))[0]


# ------------------------------------------------------------------------------------------- per-SNP terms

def test_hand_computed_snp():
    """(r1, a1, r2, a2) = (3, 1, 2, 2): pi1 = 2*1*3/(4*3), pi2 = 2*2*2/(4*3), dxy = (1*2 + 3*2)/16,
    theta_W,1 = 1 / (1 + 1/2 + 1/3)."""
    want = {"pi1": 0.5, "pi2": 2.0 / 3.0, "dxy": 0.5, "thw1": 6.0 / 11.0, "thw2": 6.0 / 11.0, "s1": 1, "s2": 1,
            "s1_full": 1, "s2_full": 1, "ar1_full": 3, "ar2_full": 4}
    t = DU.snp_terms(3, 1, 2, 2, 2, 2)
    s = _sums([(3, 1, 2, 2)])
    for f, v in want.items():
        assert close(t[f], v, rel=1e-15) and close(float(s[f]), v, rel=1e-15), (f, t[f], s[f], v)
    # not fully called at pop size 3 (n = 4 != 6): S stays, S_full and AR_full go
    s3 = _sums([(3, 1, 2, 2)], 3, 3)
    assert (s3["s1"], s3["s1_full"], s3["ar1_full"], s3["s2_full"], s3["ar2_full"]) == (1, 0, 0, 0, 0)


@pytest.mark.parametrize("snp", [(1, 0, 2, 2), (0, 1, 2, 2), (0, 0, 2, 2)], ids=["n1_ref", "n1_alt", "n0"])
def test_low_called_population_keeps_the_other(snp):
    """n = 1 or n = 0 in population 1: its pi, S and theta are 0, population 2's stay; dxy needs n1 >= 1."""
    s = _sums([snp])
    t = DU.snp_terms(*snp, 2, 2)
    assert s["pi1"] == 0.0 and s["thw1"] == 0.0 and s["s1"] == 0 and s["s1_full"] == 0 and s["ar1_full"] == 0
    assert close(float(s["pi2"]), 2.0 / 3.0, rel=1e-15) and s["s2"] == 1 and s["s2_full"] == 1 and s["ar2_full"] == 4
    r1, a1, r2, a2 = snp
    dxy = (a1 * r2 + r1 * a2) / ((r1 + a1) * (r2 + a2)) if r1 + a1 else 0.0
    assert float(s["dxy"]) == dxy == t["dxy"] == (0.5 if r1 + a1 else 0.0)
    # and in both populations: everything 0
    z = _sums([(1, 0, 0, 1)])
    assert z["pi1"] == z["pi2"] == 0.0 and z["s1"] == z["s2"] == 0 and float(z["dxy"]) == 1.0
    z = _sums([(0, 0, 0, 0), (0, 0, 1, 0)])
    assert all(float(z[f]) == 0.0 for f in DU.DOUBLES) and all(int(z[f]) == 0 for f in DU.INTS)


@pytest.mark.parametrize("fold", [False, True])
def test_fixed_alt_with_missing_calls_is_exactly_zero(fold):
    """A site fixed for the alternative allele in both populations, some calls missing: exact 0.0 everywhere
    (a r = 0 as an integer; p = a * (1/n) would not be exactly 1)."""
    s = _sums([(0, 3, 0, 2), (0, 4, 0, 3), (0, 49, 0, 27)], 25, 14, fold)
    for f in DU.DOUBLES:
        assert float(s[f]) == 0.0, f
    for f in DU.INTS:
        assert int(s[f]) == 0, f
    for snp in ((0, 3, 0, 2), (0, 49, 0, 27), (7, 0, 5, 0)):
        t = DU.snp_terms(*snp, 25, 14)
        assert all(t[f] == 0 for f in t)


def test_overcalled_snp_is_not_fully_called():
    s = _sums([(3, 2, 2, 2)], 2, 2)       # n1 = 5 > 4
    assert (s["s1"], s["s1_full"], s["ar1_full"]) == (1, 0, 0) and (s["s2"], s["s2_full"], s["ar2_full"]) == (1, 1, 4)
    assert close(float(s["pi1"]), 2 * 2 * 3 / 20.0, rel=1e-15) and close(float(s["thw1"]), 1 / (1 + 1 / 2 + 1 / 3 + 1 / 4), rel=1e-15)


def test_filters_decide_membership():
    p = _packed([(3, 1, 2, 2)] * 4, pos=[10, 20, 30, 40])
    p.ann_id[:] = [0, 1, 0, 1]
    p.ann_names = ["x", "y"]
    assert DV.window_sums(p, 0, 4, O.Cfg(2, 2, "y", False))[0]["s1"] == 2
    assert DV.window_sums(p, 0, 4, O.Cfg(2, 2, None, False, 20, 30))[0]["s1"] == 2
    assert DV.window_sums(p, 0, 4, O.Cfg(2, 2, "y", False, 20, 30))[0]["s1"] == 1
    from sfs2d.engine import ScanConfig
    assert DV.window_sums(p, 0, 4, ScanConfig(n1p=2, n2p=2, ann_want=1, start_position=20))[0]["s1"] == 2
    assert DV.window_sums(p, [0, 2, 3], [2, 4, 3], O.Cfg(2, 2))["s1"].tolist() == [2, 2, 0]


def test_window_sums_matches_the_test_helper():
    """The module's twin and the helper's own restatement agree on a genome with every awkward kind of SNP."""
    from sfs2d.synth import synth_genome
    p = synth_genome(2, [700, 300], 18, 14, seed=3, n_ann=3)
    c = p.counts.copy()
    c[5], c[64], c[65], c[128], c[699] = (pack_counts(*[np.array([v]) for v in s])[0] for s in
                                          ((0, 0, 20, 8), (1, 0, 0, 1), (0, 30, 0, 20), (40, 3, 10, 18), (36, 0, 28, 0)))
    p = PackedSNPs(c, p.pos, p.chrom_off, p.chrom_names, p.ann_id, p.ann_names)
    rng = [(0, 1), (0, 64), (3, 130), (600, 700), (700, 1000), (64, 66)]
    for cfg in (O.Cfg(18, 14), O.Cfg(18, 14, "intron_variant", False, 5000, None)):
        want = DU.expected(p, rng, cfg)
        got = DV.window_sums(p, [b for b, _ in rng], [e for _, e in rng], cfg)
        DU.assert_records(got, want)
        assert want["s1"].sum() > 0


# ------------------------------------------------------------------------------------------- Tajima's D

def test_tajima_d_values():
    # n = 10, S = 16, pi = 3.888889 (Tajima 1989's constants): AR with 2 AR / 90 = pi
    assert abs(DV.tajima_d(10, 16, 3.888889 * 90 / 2) - (-1.4461720)) <= 1e-6
    # n = 4, four sites with alt counts (1, 2, 3, 1): AR = 3 + 4 + 3 + 3
    assert abs(DV.tajima_d(4, 4, 13) - (-0.0650102495)) <= 1e-9
    assert DV.tajima_d(10, 0, 0) is None
    assert DV.tajima_d(2, 5, 5) is None and DV.tajima_d(3, 5, 5) is None


# ------------------------------------------------------------------------------------------- rows

def _genome():
    from sfs2d.synth import synth_genome
    return synth_genome(2, [500, 260], 18, 14, seed=11)


def _div_for(p, recs, cfg):
    return DU.expected_for_records(p, recs, cfg)


def test_rows_fixed_bp_labels_scaling_and_empty_slots():
    p, ocfg, W = _genome(), O.Cfg(18, 14), 150
    bgs = O.chrom_backgrounds(p, ocfg)
    recs = FR.bp_records(p, W, ocfg, lambda c: bgs[c], prev_extra=True)
    assert ((recs["flags"] & L.W_EMPTY) != 0).any() and (recs[-1]["flags"] & L.W_EXTRA)
    div = _div_for(p, recs, ocfg)
    rows = DV.rows(recs, div, p, W, "bp", pop_sizes=(18, 14))
    labels = [lb for lb in post.record_labels(recs, p, "bp", W) if lb is not None]
    assert list(rows) == labels and len(rows) == int(((recs["flags"] & (L.W_EMPTY | L.W_EXTRA)) == 0).sum())
    scan = post.combined_scan(recs, p, W, post.num_slots(recs))
    assert set(scan) <= set(rows)                      # the scan's labels, the same strings
    for lb, (b, e) in zip(labels, [(int(r["begin"]), int(r["end"])) for r in recs if not r["flags"] & (L.W_EMPTY | L.W_EXTRA)]):
        d = DU.expected(p, [(b, e)], ocfg)[0]
        r = rows[lb]
        assert list(r) == DV.KEYS
        assert r["pi_pop1"] == float(d["pi1"]) / W and r["dxy"] == float(d["dxy"]) / W
        assert r["theta_w_pop2"] == float(d["thw2"]) / W
        assert r["da"] == r["dxy"] - (r["pi_pop1"] + r["pi_pop2"]) / 2
        assert (r["S_pop1"], r["S_full_pop2"]) == (int(d["s1"]), int(d["s2_full"]))          # not scaled
        assert r["tajima_d_pop1"] == DV.tajima_d(36, d["s1_full"], d["ar1_full"])
    assert any(r["tajima_d_pop1"] is not None for r in rows.values())
    assert all(r["tajima_d_pop1"] is None for r in DV.rows(recs, div, p, W, L.WINDOW_BP).values())


def test_rows_sliding_and_snp_count_spans():
    p, ocfg = _genome(), O.Cfg(18, 14)
    bgs = O.chrom_backgrounds(p, ocfg)
    # sliding: labels advance by the step, the divisor is the window
    W, step = 8000, 2000
    recs = FR.bp_records(p, step, ocfg, lambda c: bgs[c])          # slot j = records of wid j (ranges irrelevant here)
    div = _div_for(p, recs, ocfg)
    rows = DV.rows(recs, div, p, W, "bp", step)
    assert list(rows) == [lb for lb in post.record_labels(recs, p, "bp", W, step) if lb is not None]
    assert list(rows) == list(post.sliding_scan(recs, p, W, step))
    live = recs[(recs["flags"] & L.W_EMPTY) == 0]
    d0 = DU.expected(p, [(int(live[0]["begin"]), int(live[0]["end"]))], ocfg)[0]
    assert next(iter(rows.values()))["pi_pop2"] == float(d0["pi2"]) / W
    # SNP-count windows: first to last position of the window's SNPs
    S = 64
    recs = FR.snp_records(p, S, ocfg, lambda c: bgs[c])
    div = _div_for(p, recs, ocfg)
    rows = DV.rows(recs, div, p, S, "snps", pop_sizes=(18, 14))
    assert list(rows) == list(post.bysnp_scan(recs, p, S, True, False))
    for r, d, row in zip(recs, div, rows.values()):
        span = int(p.pos[int(r["end"]) - 1]) - int(p.pos[int(r["begin"])]) + 1
        assert row["pi_pop1"] == float(d["pi1"]) / span and row["theta_w_pop1"] == float(d["thw1"]) / span
        assert row["S_pop1"] == int(d["s1"])
    with pytest.raises(ValueError):
        DV.rows(recs, div[:-1], p, S, "snps")


# ------------------------------------------------------------------------------------------- CSV

def _stats(with_div, with_p):
    row = {"snp_count": 5, "T2D": 1.5, "T1D_pop1": 0.5, "T1D_pop2": None, "new_term_pop1": 1.0, "new_term_pop2": None,
           "T2D_diff": None}
    if with_div:
        row.update({k: 0.25 for k in DV.KEYS})
        row["S_pop1"], row["tajima_d_pop2"] = 7, None
    if with_p:
        row.update({k: 0.5 for k in cli.P_COLS})
    return {"c1 1-1000": row}


@pytest.mark.parametrize("fst", [False, True])
@pytest.mark.parametrize("null", [False, True])
def test_csv_column_order(tmp_path, fst, null):
    import twoDSFS_class as T
    path = str(tmp_path / "o.csv")
    cli.write_csv(path, _stats(True, null), {}, {"c1 1-1000": 0.125} if fst else None, None, null, diversity=True)
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    assert list(rows[0]) == T.col_names + (["FST"] if fst else []) + DV.KEYS + (cli.P_COLS if null else [])
    assert rows[0]["S_pop1"] == "7" and rows[0]["pi_pop1"] == "0.25"
    assert rows[0]["tajima_d_pop2"] == "" == rows[0]["T1D_p2"]          # None: the CSV's empty field


@pytest.mark.parametrize("fst", [False, True])
@pytest.mark.parametrize("null", [False, True])
def test_csv_without_diversity_is_unchanged(tmp_path, fst, null):
    """Rows that carry the diversity keys or not: without the flag the file is the one written before."""
    import twoDSFS_class as T
    f = {"c1 1-1000": 0.125} if fst else None
    a, b = str(tmp_path / "a.csv"), str(tmp_path / "b.csv")
    cli.write_csv(a, _stats(False, null), {}, f, None, null)
    cli.write_csv(b, _stats(True, null), {}, f, None, null, diversity=False)
    assert open(a, "rb").read() == open(b, "rb").read()
    with open(a, newline="") as fh:
        assert next(csv.reader(fh)) == T.col_names + (["FST"] if fst else []) + (cli.P_COLS if null else [])


def test_cli_passes_diversity_only_with_the_flag(monkeypatch, tmp_path):
    """The CLI through a stubbed class: --diversity reaches multi_scan / scan_pvalues and write_csv; without it
    the calls carry no such keyword (byte-identical behaviour)."""
    import twoDSFS_class as T
    import sfs2d.vcf as V
    calls = []

    class Stub:
        def __init__(self, *a, **k):
            pass

        def multi_scan(self, packed, ws, snps, **kw):
            calls.append(("multi_scan", kw))
            return {w: _stats(kw.get("diversity", False), False) for w in ws}

        def scan_pvalues(self, packed, ws, snps=(), **kw):
            calls.append(("scan_pvalues", kw))
            return {w: _stats(kw.get("diversity", False), True) for w in ws}

    monkeypatch.setattr(T, "LikelihoodInference_jointSFS", Stub)
    monkeypatch.setattr(V, "make_packed_vcf", lambda *a, **k: type("P", (), {"n": 0, "nchrom": 0})())
    heads = {}
    for name, extra in (("plain", []), ("div", ["--diversity"]), ("divnull", ["--diversity", "--null-replicates", "9"])):
        outs = cli.main(["x.vcf", "pm.txt", "--window", "1000", "--out-prefix", str(tmp_path / name)] + extra)
        with open(outs[0], newline="") as fh:
            heads[name] = next(csv.reader(fh))
    assert "diversity" not in calls[0][1] and calls[1][1]["diversity"] is True and calls[2][1]["diversity"] is True
    assert calls[2][0] == "scan_pvalues"
    assert heads["plain"] == T.col_names
    assert heads["div"] == T.col_names + DV.KEYS
    assert heads["divnull"] == T.col_names + DV.KEYS + cli.P_COLS


def test_distributed_diversity_is_refused():
    import twoDSFS_class as T
    obj = T.LikelihoodInference_jointSFS(None, None, distributed=True)
    p = _genome()
    for call in (lambda: obj.multi_scan(p, [20000], diversity=True), lambda: obj.sliding_scan(p, 20000, 5000, diversity=True),
                 lambda: obj.multi_sliding_scan(p, [20000], 5000, diversity=True),
                 lambda: obj.scan_pvalues(p, [20000], diversity=True), lambda: obj.window_diversity(p, 20000)):
        with pytest.raises(NotImplementedError, match="diversity"):
            call()


# ------------------------------------------------------------------------------------------- layout

def test_diversity_dtype_matches_the_header():
    src = open(os.path.join(REPO, "include", "sfs2d.h")).read()
    body = src[:src.index("} sfs2d_diversity;")]
    body = body[body.rindex("typedef struct {"):]
    ctype = {"double": "<f8", "uint64_t": "<u8", "uint32_t": "<u4"}
    fields = []
    for t, names in re.findall(r"^\s*(double|uint64_t|uint32_t)\s+([\w,\s]+);", body, re.M):
        fields += [(n.strip(), ctype[t]) for n in names.split(",")]
    assert fields[0][1] == "<f8"                       # the first member is a double
    assert [(n, L.DIVERSITY_DTYPE.fields[n][0].str) for n in L.DIVERSITY_DTYPE.names] == fields
    assert L.DIVERSITY_DTYPE.itemsize == 80 == sum(np.dtype(t).itemsize for _, t in fields)
    assert [L.DIVERSITY_DTYPE.fields[n][1] for n in L.DIVERSITY_DTYPE.names] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72, 76]
    assert "sfs2d_plan_diversity" in L.EXPORTS and "sfs2d_plan_diversity_read" in L.EXPORTS
