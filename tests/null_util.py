"""Shared by the bootstrap-null tests: oracle-evaluated twins of the device's null records."""
import numpy as np

from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import null as N


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


def ks_uniform(pv):
    """Kolmogorov-Smirnov distance of a sample to U(0, 1)."""
    x = np.sort(np.asarray(pv, float))
    n = len(x)
    i = np.arange(1, n + 1)
    return float(max(np.max(i / n - x), np.max(x - (i - 1) / n)))
