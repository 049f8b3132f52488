"""The dynamic-LDS limit of a kernel family only grows (grant_lds; DESIGN.md, "kernel variants"): a plan that needs
less dynamic LDS than an earlier plan on the same device must not lower the limit under the earlier plan's launches.
Each test runs plan A, then a plan B of the same family that needs less -- both above the default 65,536 B -- then A
again, and checks every result.  Small data: two chromosomes of 2,000 and 1,900 SNPs; only the grids are
large."""
import pytest

import spectra_util as SU
from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import spectra as SP

pytestmark = pytest.mark.gpu

LENGTHS = [2000, 1900]
WHOLE = 10_000_000        # bp: every chromosome is one window (the spectra test)
W = 20000                 # bp: ~6 windows per chromosome (the scan test: a window that is its chromosome has T2D 0)


def _cfg(n1p, n2p, window):
    from sfs2d.engine import ScanConfig
    return ScanConfig(n1p=n1p, n2p=n2p, window=window, bg_mode=L.BG_PER_CHROM)


def test_spectra_rows_of_two_plans_above_the_default_limit():
    """k_spec_win's row as a u32 histogram in LDS, 4 x SFS2D_SPEC_ROW_WORDS bytes: plan A at 100 / 75 takes
    4 x (201 x 151 + 100 + 75 + 2) = 122,112 B, plan B at 65 / 65 takes 4 x (131 x 131 + 65 + 65 + 2) = 69,172 B."""
    a, b = (100, 75), (65, 65)
    assert 4 * L.spec_row_words(*a) == 122112 and 4 * L.spec_row_words(*b) == 69172
    pa, pb = (SU.genome(*s, lengths=LENGTHS, plant=False) for s in (a, b))
    ca, cb = _cfg(*a, WHOLE), _cfg(*b, WHOLE)
    with SU.Run(pa, ca) as ra, SU.Run(pb, cb) as rb:
        want_a = SP.window_spectra_np(pa, ra.pl.read(), ca)
        want_b = SP.window_spectra_np(pb, rb.pl.read(), cb)
        assert want_a.shape == (2, L.spec_row_words(*a)) and want_a.sum() > 3000 and want_b.sum() > 3000
        first = ra.pl.spectra()
        got_b = rb.pl.spectra()
        again = ra.pl.spectra()
    SU.assert_rows(first, want_a, "A, first")
    SU.assert_rows(got_b, want_b, "B")
    SU.assert_rows(again, want_a, "A, after B")


def _scan_w_lds(n1p, n2p):
    """plan_create's dynamic LDS of k_scan_w for a counts plan without Fst whose windows hold < 65,536 SNPs (P16):
    doubles -- the lp table (nt entries, even-rounded), D (512) and x ln x (256) -- then eight wavefronts'
    histogram blocks of [packed 2D bins, rounded to 4 | 4 x (n1p + 1) | 4 x (n2p + 1)] words, rounded to 4."""
    nb2 = (2 * n1p + 1) * (2 * n2p + 1)
    nt = nb2 + n1p + 1 + n2p + 1
    h2w = ((nb2 + 1) // 2 + 3) & ~3
    per = (h2w + 4 * (n1p + 1) + 4 * (n2p + 1) + 3) & ~3
    hist = max(8 * per, 2 * (1536 + 256) + 16 + nt + 16)
    return 8 * (((nt + 1) & ~1) + 512 + 256) + 4 * hist


def test_scans_of_two_plans_above_the_default_limit():
    """k_scan_w: plan A at 25 / 25 (the 51 x 51 grid) launches with 75,760 B of dynamic LDS, plan B at 24 / 24 with
    70,688 B (with Fst the headline configuration's 81,776 B; these plans ask for none)."""
    a, b = (25, 25), (24, 24)
    assert _scan_w_lds(*a) == 75760 and _scan_w_lds(*b) == 70688
    pa, pb = (SU.genome(*s, lengths=LENGTHS, plant=False) for s in (a, b))
    with SU.Run(pa, _cfg(*a, W), run=False) as ra, SU.Run(pb, _cfg(*b, W), run=False) as rb:
        out = []
        for r in (ra, rb, ra):
            r.pl.run()
            r.pl.check()
            assert r.pl.scan_kernel() == "k_scan_w" and r.pl.scan_variant()["cnt"] == 1
            out.append(r.pl.read())
    assert out[0].tobytes() == out[2].tobytes()
    for p, s, recs in ((pa, a, out[0]), (pb, b, out[1])):
        ocfg = O.Cfg(*s)
        bgs = O.chrom_backgrounds(p, ocfg)
        ref = O.window_records(p, O.bp_windows(p, W), ocfg, lambda c: bgs[c])
        recs = recs[(recs["flags"] & L.W_EMPTY) == 0]
        assert len(ref) == len(recs) >= 10
        nt = 0
        for r, o in zip(recs, ref):
            for f, g in (("snp_count", "snp_count"), ("n2", "N2"), ("n1a", "N1a"), ("n1b", "N1b")):
                assert int(r[f]) == o[g], (s, f, int(r[f]), o[g])
            for f, g in (("t2d", "T2D"), ("t1d_p1", "T1D_p1"), ("t1d_p2", "T1D_p2")):
                if o[g] is not None:   # (the tolerance of the build's own end-to-end check)
                    assert abs(float(r[f]) - o[g]) <= 1e-10 * max(abs(o[g]), 1e-300), (s, f, float(r[f]), o[g])
                    nt += 1
        assert nt >= 30
