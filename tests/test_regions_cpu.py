"""Region windows, the parts that need no GPU: the BED reader, the Regions value (stable sort by chromosome and the
permutation back), the numpy definition of a region's SNP range against hand-written literals, post.region_scan's
rows on fake records (one row per region, empty ones included, the caller's order), ScanConfig.regions, and the
argument errors of the class methods and the CLI, raised before an engine is made."""
import types

import numpy as np
import pytest

import fake_records
import twoDSFS_class as T
from sfs2d import _lib as L
from sfs2d import cli, diversity, post
from sfs2d.engine import ScanConfig
from sfs2d.regions import Regions, read_bed, region_ranges

KEYS = ["snp_count", "T2D", "T1D_pop1", "T1D_pop2", "new_term_pop1", "new_term_pop2", "T2D_diff"]


def _bed(tmp_path, text, name="r.bed"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_read_bed_coordinates_comments_names(tmp_path):
    path = _bed(tmp_path, "# genes\ntrack name=genes\nbrowser position chrA:1-100\n\n"
                          "chrA\t0\t100\tgeneA\t0\t+\nchrB\t99\t100\nchrA 10 20 spaced\nchrA\t5\t6\t.\n")
    # 0-based half-open -> 1-based inclusive: first = start + 1, last = end; column 4 is the name
    assert read_bed(path) == [("chrA", 1, 100, "geneA"), ("chrB", 100, 100), ("chrA", 11, 20, "spaced"), ("chrA", 6, 6)]


@pytest.mark.parametrize("line, what", [("chrA\t100\t100\n", "start < end"), ("chrA\t7\t3\n", "start < end"),
                                        ("chrA\t-1\t3\n", "start < end"), ("chrA\tx\t3\n", "invalid literal"),
                                        ("chrA\t5\n", "fewer than 3 columns")])
def test_read_bed_bad_line(tmp_path, line, what):
    path = _bed(tmp_path, "chrA\t0\t10\n# comment\n" + line)
    with pytest.raises(ValueError, match="line 3") as ei:
        read_bed(path)
    assert what in str(ei.value)


def test_regions_sort_and_inverse_permutation():
    names = ["chrA", "chrB", "chrC"]
    items = [("chrC", 5, 9), ("chrA", 100, 200, "g1"), ("chrC", 1, 3), ("chrA", 50, 60), ("chrA", 100, 200, "g2"),
             ("chrB", 0, (1 << 32) - 1)]
    rg = Regions(names, items)
    assert len(rg) == 6
    # stable by chromosome: a chromosome's regions keep the caller's order among themselves
    assert rg.order.tolist() == [1, 3, 4, 5, 0, 2]
    assert rg.chrom.tolist() == [0, 0, 0, 1, 2, 2] and rg.chrom.dtype == np.int32
    assert rg.first.tolist() == [100, 50, 100, 0, 5, 1] and rg.first.dtype == np.uint32
    assert rg.last.tolist() == [200, 60, 200, (1 << 32) - 1, 9, 3] and rg.last.dtype == np.uint32
    assert rg.slot.tolist() == [4, 0, 5, 1, 2, 3]
    assert all(rg.order[rg.slot[i]] == i for i in range(6))
    assert rg.keys() == ["chrC 5-9", "g1", "chrC 1-3", "chrA 50-60", "g2", "chrB 0-4294967295"]
    assert rg.slot_keys() == ["g1", "chrA 50-60", "g2", "chrB 0-4294967295", "chrC 5-9", "chrC 1-3"]
    assert rg.lengths().tolist() == [101, 11, 101, 1 << 32, 5, 3]
    assert rg.names == [None, "g1", None, None, "g2", None]


def test_regions_errors():
    names = ["chrA", "chrB"]
    with pytest.raises(ValueError, match="'chrZ'"):
        Regions(names, [("chrA", 1, 2), ("chrZ", 1, 2)])
    with pytest.raises(ValueError, match="duplicate region key 'chrA 1-2'"):
        Regions(names, [("chrA", 1, 2), ("chrB", 1, 2), ("chrA", 1, 2)])
    with pytest.raises(ValueError, match="duplicate region key 'g'"):
        Regions(names, [("chrA", 1, 2, "g"), ("chrB", 5, 9, "g")])
    Regions(names, [("chrA", 1, 2, "g"), ("chrA", 1, 2, "h")])   # an identical pair, named apart
    for bad in ([("chrA", 3, 2)], [("chrA", -1, 2)], [("chrA", 1, 1 << 32)], [("chrA", 1)], []):
        with pytest.raises(ValueError):
            Regions(names, bad)
    p = types.SimpleNamespace(chrom_names=["chrA"])
    with pytest.raises(ValueError, match="another data set"):
        Regions.of(p, Regions(names, [("chrA", 1, 2)]))
    assert Regions.of(p, [("chrA", 1, 2)]).keys() == ["chrA 1-2"]


def test_region_ranges_literals():
    """A 12-SNP chromosome (SNPs 3 .. 14 of the data set) with a repeated position and a SNP at position 0, between
    a 3-SNP chromosome and an empty one."""
    pos = np.array([5, 6, 7,   0, 3, 3, 3, 10, 11, 20, 20, 21, 40, 41, 99], np.uint32)
    p = types.SimpleNamespace(pos=pos, chrom_off=np.array([0, 3, 15, 15], np.int64), chrom_names=["a", "b", "c"])
    cases = [(("b", 0, 0), (3, 4)),            # first == 0: the SNP at position 0
             (("b", 1, 2), (4, 4)),            # empty: between position 0 and the first 3
             (("b", 1, 3), (4, 7)),            # last on a repeated position: all three copies
             (("b", 3, 3), (4, 7)),            # first and last on it
             (("b", 3, 10), (4, 8)),
             (("b", 4, 9), (7, 7)),            # empty: between two neighbouring SNPs
             (("b", 1, 99), (4, 15)),          # the chromosome without its position-0 SNP
             (("b", 0, (1 << 32) - 1), (3, 15)),   # last + 1 = 2^32
             (("b", 20, 20), (9, 11)),
             (("b", 21, 40), (11, 13)),
             (("b", 100, 200), (15, 15)),      # empty: after the last SNP
             (("b", 99, 99), (14, 15)),        # the last SNP alone
             (("a", 6, 6), (1, 2)),
             (("a", 8, (1 << 32) - 1), (3, 3)),    # empty; must not run into chromosome b
             (("c", 1, 1000), (15, 15))]       # a chromosome without SNPs
    rg = Regions(p.chrom_names, [c[0] for c in cases])
    begin, end = region_ranges(p, rg)
    got = {k: (int(begin[s]), int(end[s])) for k, s in zip(rg.keys(), rg.slot.tolist())}
    want = {f"{c} {f}-{l}": r for (c, f, l), r in cases}
    assert got == want


def _fake():
    """Six regions on two chromosomes, the caller's order mixing them; slot order: chrA (g_full, g_empty, g_n1a),
    chrB (g_bg0, g_zero, g_empty2)."""
    packed = types.SimpleNamespace(chrom_names=["chrA", "chrB"])
    rg = Regions(packed.chrom_names, [("chrB", 1, 50, "g_bg0"), ("chrA", 1, 100, "g_full"), ("chrA", 200, 300),
                                      ("chrB", 60, 70, "g_zero"), ("chrA", 50, 250, "g_n1a"), ("chrB", 900, 901)])
    recs = np.zeros(6, dtype=L.WINDOW_DTYPE)
    o = dict(snp_count=9, N2=5, N2_all=6, N1a=3, N1b=2, T2D=10.0, T1D_p1=4.0, T1D_p2=2.0)
    for k, c in enumerate(rg.chrom.tolist()):
        r = recs[k]
        fake_records._fill(r, o)
        r["chrom"], r["wid"], r["begin"], r["end"] = c, k % 3, 10 * k, 10 * k + 9
        recs[k] = r
    for k in (1, 5):   # "chrA 200-300" and "chrB 900-901" hold no SNP
        recs[k] = np.zeros((), L.WINDOW_DTYPE)
        recs[k]["flags"] = L.W_EMPTY
        recs[k]["chrom"], recs[k]["wid"] = rg.chrom[k], k % 3
    recs[2]["n1a"] = 0
    recs[3]["flags"] = L.W_BG2_ZERO
    recs[4]["t2d"] = 0.0
    return recs, packed, rg


def test_region_scan_rows_order_and_empty_rows():
    recs, packed, rg = _fake()
    rows = post.region_scan(recs, packed, rg)
    # one row per region, in the caller's order, the unnamed ones keyed "<chrom> <first>-<last>"
    assert list(rows) == ["g_bg0", "g_full", "chrA 200-300", "g_zero", "g_n1a", "chrB 900-901"]
    assert all(list(r) == KEYS for r in rows.values())
    assert rows["g_full"] == dict(zip(KEYS, [9, 10.0, 4.0, 2.0, 6.0, 8.0, 7.0]))
    # a region without SNPs is a row: snp_count 0, every statistic None
    assert rows["chrA 200-300"] == rows["chrB 900-901"] == dict(zip(KEYS, [0] + [None] * 6))
    assert rows["g_n1a"] == dict(zip(KEYS, [9, 10.0, None, 2.0, None, 8.0, None]))
    assert rows["g_bg0"] == dict(zip(KEYS, [9, None, 4.0, 2.0, None, None, None]))
    assert rows["g_zero"] == dict(zip(KEYS, [9, 0.0, 4.0, 2.0, -4.0, -2.0, -3.0]))
    fst = np.array([0.25, np.nan, np.nan, 0.5, -0.125, np.nan])   # slot order
    rows = post.region_scan(recs, packed, rg, fst)
    assert all(list(r) == KEYS + ["FST"] for r in rows.values())
    assert [r["FST"] for r in rows.values()] == [0.5, 0.25, None, -0.125, None, None]
    assert post.region_labels(recs, rg) == ["g_full", None, "g_n1a", "g_bg0", "g_zero", None]
    with pytest.raises(ValueError):
        post.region_scan(recs[:5], packed, rg)


def test_diversity_rows_divide_by_the_regions_length():
    recs, packed, rg = _fake()
    div = np.zeros(6, L.DIVERSITY_DTYPE)
    div["pi1"], div["pi2"], div["dxy"], div["thw1"], div["s1"] = 5.0, 1.0, 4.0, 2.0, 7
    rows = diversity.rows(recs, div, packed, None, None, regions=rg)
    assert sorted(rows) == sorted(rg.keys())
    full = rows["g_full"]    # chrA 1-100: 100 sites
    assert (full["pi_pop1"], full["pi_pop2"], full["dxy"], full["theta_w_pop1"]) == (0.05, 0.01, 0.04, 0.02)
    assert full["da"] == 0.04 - (0.05 + 0.01) / 2 and full["S_pop1"] == 7 and full["tajima_d_pop1"] is None
    assert rows["g_n1a"]["pi_pop1"] == 5.0 / 201    # chrA 50-250
    assert rows["chrA 200-300"] == dict.fromkeys(diversity.KEYS)   # an empty region: twelve None
    stats = post.region_scan(recs, packed, rg)
    diversity.add_columns(stats, recs, div, packed, None, None, regions=rg)
    assert all(list(r) == KEYS + diversity.KEYS for r in stats.values())


def test_scan_config_regions():
    import dataclasses
    rg = Regions(["chrA"], [("chrA", 1, 2)])
    assert "regions" in [f.name for f in dataclasses.fields(ScanConfig)]
    a = ScanConfig(n1p=18, n2p=14, fst=True)
    b = ScanConfig(n1p=18, n2p=14, fst=True, regions=rg)
    assert a.regions is None and b.regions is rg
    assert bytes(a.params()) == bytes(b.params())   # the list is an argument of the regions entry points
    with pytest.raises(ValueError, match="exclusive"):
        ScanConfig(n1p=18, n2p=14, regions=rg, step=5000)


def _packed():
    from sfs2d.synth import synth_genome
    return synth_genome(2, [30, 20], 18, 14, seed=5)


def test_class_methods_check_their_arguments_first(monkeypatch, tmp_path):
    """An unknown chromosome, first > last, a duplicate key, a bad BED line, an unknown background chromosome:
    ValueError before an engine is made (none can be made here)."""
    made = []
    monkeypatch.setattr(T.Engine, "get", classmethod(lambda cls, device=0: made.append(device)))
    p = _packed()
    obj = T.LikelihoodInference_jointSFS(None, None, pop1=p.pop1, pop2=p.pop2)
    c0 = p.chrom_names[0]
    bad_bed = _bed(tmp_path, f"{c0}\t10\t10\n")
    for bad in ([("nope", 1, 2)], [(c0, 9, 2)], [(c0, 1, 2), (c0, 1, 2)], bad_bed, []):
        with pytest.raises(ValueError):
            obj.region_scan(p, bad)
        with pytest.raises(ValueError):
            obj.multi_scan(p, [20000], regions=bad)
        with pytest.raises(ValueError):
            obj.multi_sliding_scan(p, [20000], 5000, regions=bad)
        with pytest.raises(ValueError):
            obj.scan_pvalues(p, [20000], regions=bad, replicates=9)
    with pytest.raises(ValueError, match="'nope'"):
        obj.region_scan(p, [("nope", 1, 2)])
    with pytest.raises(ValueError, match="Background chromosome nope not found in the data."):
        obj.region_scan(p, [(c0, 1, 2)], background_chromosome="nope")
    with pytest.raises(ValueError, match="no window sizes"):
        obj.scan_pvalues(p, [20000], regions=[(c0, 1, 2)], background_chromosome=c0, replicates=9)
    assert made == []


def test_distributed_is_not_implemented():
    p = _packed()
    obj = T.LikelihoodInference_jointSFS(None, None, distributed=True)
    rg = [(p.chrom_names[0], 1, 2)]
    with pytest.raises(NotImplementedError):
        obj.region_scan(p, rg)
    with pytest.raises(NotImplementedError):
        obj.multi_scan(p, [20000], regions=rg)
    with pytest.raises(NotImplementedError):
        obj.multi_sliding_scan(p, [20000], 5000, regions=rg)
    with pytest.raises(NotImplementedError):
        obj.scan_pvalues(p, [20000], regions=rg, replicates=9)


def test_cli_help_names_the_flag(capsys):
    with pytest.raises(SystemExit) as ei:
        cli.main(["--help"])
    assert ei.value.code == 0
    assert "--regions FILE.bed" in capsys.readouterr().out
