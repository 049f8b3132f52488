"""Shared by the bootstrap-null tests: oracle-evaluated twins of the device's null records."""
import numpy as np

import golden_util as gu
from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import null as N

INTS = ("chrom", "wid", "begin", "end", "snp_count", "n2", "n2_all", "n1a", "n1b", "flags")
T_FLOOR = 1e-2   # T's below it are compared as if they were 1e-2 (test_null_gpu.py's module docstring)


def oracle_records(p, wins, cfg, bg_of, chrom_of=lambda w: w[0], wid_of=lambda w: w[1]):
    """oracle.window_records of ``wins`` ((c, ..., begin, end) tuples over p) as WINDOW_DTYPE records:
    chrom / wid from the tuple, begin = 0 and end = the SNP count (a null record's layout), the counts, the
    T's, and a BG-zero flag exactly where the oracle returns None although the window's N is not 0."""
    ref = O.window_records(p, wins, cfg, bg_of)
    out = np.zeros(len(wins), L.WINDOW_DTYPE)
    for r, w, o in zip(out, wins, ref):
        r["chrom"] = chrom_of(w) & 0xFFFFFFFF
        r["wid"] = wid_of(w)
        r["end"] = w[-1] - w[-2]
        for f, g in (("snp_count", "snp_count"), ("n2", "N2"), ("n2_all", "N2_all"), ("n1a", "N1a"), ("n1b", "N1b")):
            r[f] = o[g]
        bg2, bg1a, bg1b = bg_of(w[0])
        zero = (sum(np.asarray(bg2).ravel()[1:-1].tolist()) == 0, sum(np.asarray(bg1a)[1:cfg.n1p].tolist()) == 0,
                sum(np.asarray(bg1b)[1:cfg.n2p].tolist()) == 0)
        fl = 0
        for f, g, n, z, bz in (("t2d", "T2D", "N2", L.W_BG2_ZERO, zero[0]), ("t1d_p1", "T1D_p1", "N1a", L.W_BG1A_ZERO, zero[1]),
                               ("t1d_p2", "T1D_p2", "N1b", L.W_BG1B_ZERO, zero[2])):
            assert (o[g] is None) == (o[n] == 0 or bz), (w, g, o)   # the record's validity rule is the oracle's None
            if bz:
                fl |= z
            if o[g] is not None:
                r[f] = o[g]
        r["flags"] = fl
    return out


def null_twin(p, tasks, replicates, seed, cfg, bg_of):
    """The records Plan.null_run(tasks, replicates, seed) should write, from the host twin of the draws
    and the oracle: (records, replicate data set, windows)."""
    q, wins = N.resample(p, tasks, replicates, seed)
    return oracle_records(q, wins, cfg, bg_of), q, wins


def check(got, want, wide=False):
    """wide (windows of 65,536 SNPs): S and N ln N are ~3e5 there, each a sum of tens of rounded terms, so
    either side's absolute error is up to ~100 eps N ln N = 3e-9 (seen: 7e-11 on T1D = 0.18): the relative
    1e-10 is then taken of max(|T|, 1e-4 N ln N)."""
    assert len(got) == len(want) > 0
    for f in INTS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, (f, bad[:5], got[f][bad[:5]], want[f][bad[:5]], got[["chrom", "wid", "end"]][bad[:5]])
    assert np.array_equal(N.valid_mask(got), N.valid_mask(want))
    v = N.valid_mask(want)
    nvalid = 0
    for s, (f, nf) in enumerate((("t2d", "n2"), ("t1d_p1", "n1a"), ("t1d_p2", "n1b"))):
        for i in np.nonzero(v[s])[0]:
            n = float(want[nf][i])
            scale = max(T_FLOOR, 1e-4 * n * np.log(n)) if wide else T_FLOOR
            assert gu.close(float(got[f][i]), float(want[f][i]), scale=scale), (f, i, got[i], want[i])
            nvalid += 1
    return nvalid


def ks_uniform(pv):
    """Kolmogorov-Smirnov distance of a sample to U(0, 1)."""
    x = np.sort(np.asarray(pv, float))
    n = len(x)
    i = np.arange(1, n + 1)
    return float(max(np.max(i / n - x), np.max(x - (i - 1) / n)))
