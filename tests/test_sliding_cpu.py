"""Sliding windows, the parts that need no GPU: post.sliding_scan's rows, ScanConfig.step, the CLI's
--step argument errors and multi_sliding_scan's step check (raised before an engine is made)."""
import types

import numpy as np
import pytest

import fake_records
import twoDSFS_class as T
from sfs2d import _lib as L
from sfs2d import cli, post
from sfs2d.engine import ScanConfig

WS, STEP = 20000, 5000
KEYS = ["snp_count", "T2D", "T1D_pop1", "T1D_pop2", "new_term_pop1", "new_term_pop2", "T2D_diff"]


def _records():
    """Five slots of two chromosomes: a full window, an empty slot, a window without pop-1 1D SNPs, one whose
    2D background is empty, and one whose T2D is exactly 0.0."""
    recs = np.zeros(5, dtype=L.WINDOW_DTYPE)
    o = dict(snp_count=9, N2=5, N2_all=6, N1a=3, N1b=2, T2D=10.0, T1D_p1=4.0, T1D_p2=2.0)
    for k, (c, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 0), (1, 3)]):
        r = recs[k]
        fake_records._fill(r, o)
        r["chrom"], r["wid"], r["begin"], r["end"] = c, j, 10 * k, 10 * k + 9
        recs[k] = r
    recs[1]["flags"] = L.W_EMPTY
    recs[2]["n1a"] = 0
    recs[3]["flags"] = L.W_BG2_ZERO
    recs[4]["t2d"] = 0.0
    return recs, types.SimpleNamespace(chrom_names=["chrA", "chrB"])


def test_rows_labels_and_none_rules():
    recs, packed = _records()
    rows = post.sliding_scan(recs, packed, WS, STEP)
    # labels "<chrom> <j S + 1>-<j S + W>", empty slots omitted, slot order
    assert list(rows) == ["chrA 1-20000", "chrA 10001-30000", "chrB 1-20000", "chrB 15001-35000"]
    assert all(list(r) == KEYS for r in rows.values())
    assert rows["chrA 1-20000"] == dict(zip(KEYS, [9, 10.0, 4.0, 2.0, 6.0, 8.0, 7.0]))
    # N == 0 for pop 1: its T1D and what derives from it are None, the rest stays
    assert rows["chrA 10001-30000"] == dict(zip(KEYS, [9, 10.0, None, 2.0, None, 8.0, None]))
    # an empty 2D background: T2D None, every derived term None (no TypeError)
    assert rows["chrB 1-20000"] == dict(zip(KEYS, [9, None, 4.0, 2.0, None, None, None]))
    # an exact 0.0 is a value: its own derived terms, no stale carry from the window before (Q6)
    assert rows["chrB 15001-35000"] == dict(zip(KEYS, [9, 0.0, 4.0, 2.0, -4.0, -2.0, -3.0]))


def test_rows_fst_key():
    recs, packed = _records()
    fst = np.array([0.25, np.nan, np.nan, 0.5, -0.125])
    rows = post.sliding_scan(recs, packed, WS, STEP, fst)
    assert all(list(r) == KEYS + ["FST"] for r in rows.values())
    assert [r["FST"] for r in rows.values()] == [0.25, None, 0.5, -0.125]
    assert all("FST" not in r for r in post.sliding_scan(recs, packed, WS, STEP).values())


def test_step_equal_to_window_labels_as_combined_scan():
    recs, packed = _records()
    assert list(post.sliding_scan(recs, packed, WS, WS)) == [
        "chrA 1-20000", "chrA 40001-60000", "chrB 1-20000", "chrB 60001-80000"]


def test_scan_config_step():
    import dataclasses
    assert [f.name for f in dataclasses.fields(ScanConfig)][-1] == "step"
    a = ScanConfig(n1p=18, n2p=14, window=WS, fst=True)
    b = ScanConfig(n1p=18, n2p=14, window=WS, fst=True, step=STEP)
    assert a.step is None and b.step == STEP
    assert bytes(a.params()) == bytes(b.params())   # the step is an argument of the sliding entry points


@pytest.mark.parametrize("argv", [["--window", "20000", "--step", "5000", "--snp-window", "500"],
                                  ["--window", "20000", "--step", "3000"],
                                  ["--window", "20000", "--window", "50000", "--step", "20000"],
                                  ["--window", "20000", "--step", "0"],
                                  ["--window", "20000", "--step", "100"]])
def test_cli_step_argument_errors(argv, capsys):
    """--step with --snp-window, a step that does not divide every window, a step below 1 or window / 64:
    argparse errors (exit status 2), before the VCF is opened."""
    with pytest.raises(SystemExit) as ei:
        cli.main(["no_such.vcf.gz", "no_such_popmap.txt"] + argv)
    assert ei.value.code == 2
    assert "--step" in capsys.readouterr().err


def test_multi_sliding_scan_checks_the_step_first(monkeypatch):
    """A window the step does not divide: ValueError before an engine is made (none can be made here)."""
    made = []
    monkeypatch.setattr(T.Engine, "get", classmethod(lambda cls, device=0: made.append(device)))
    obj = T.LikelihoodInference_jointSFS(None, None)
    for windows, step in (([20000, 50000], 20000), ([20000], 3000), ([20000], 0), ([20000], 100)):
        with pytest.raises(ValueError):
            obj.multi_sliding_scan({}, windows, step)
        with pytest.raises(ValueError):
            obj.sliding_scan({}, windows[-1], step)
    assert made == []


def test_distributed_is_not_implemented():
    obj = T.LikelihoodInference_jointSFS(None, None, distributed=True)
    with pytest.raises(NotImplementedError):
        obj.sliding_scan({}, 20000, 5000)
    with pytest.raises(NotImplementedError):
        obj.multi_sliding_scan({}, [20000], 5000)
