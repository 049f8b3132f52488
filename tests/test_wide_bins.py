"""The scan kernels' 32-bit-bin instantiations (P16 = false) against the oracle, window by window.

plan_create packs two 2D bins per LDS word only when it can prove that no window holds 65,536 SNPs.  Data handed
over with sfs2d_data_wrap_device has no host copy of the positions, so every fixed-bp window above 65,535 bp and
every sliding plan on it takes P16 = false whatever the data holds: that is the route these cases use, at
~9,000 SNPs.  Every case runs the plan on wrapped data, asserts Plan.scan_variant() (the template arguments the
launch recorded) against the tuple written in its table, compares every record and Fst with the oracle
(wide_util.check_records: integers exact, T by golden_util.close, Fst within 1e-12 + 1e-10 |x|), then runs the same
ScanConfig on uploaded data, where the positions prove P16 = true, and asserts that the two tables agree in every
integer field and flag.

The P16 = false instantiations launch_scan / launch_scan_any can select (sfs2d.hip), all asserted below:

  k_scan_w<false, FUSED, FST, CNT, GATE>      (FUSED 1: SFS2D_FUSED=1; 0: SFS2D_FUSED=0 or a supplied background)
    Fst in the scan (counts plans):  <F, 2, 1, 1>  folded, called counts within 2 pop_size        fst_gate, wgs1, bgsup_int
                                     <F, 2, 1, 0>  unfolded / over-called data                    fst_unfold, fst_over
                                     <F, 3, 1, 1>  data with < 2 called alleles, folded           fst_mask_gate
                                     <F, 3, 1, 0>  the same, unfolded                             fst_mask_nogate
      (25 x 25 and 18 x 14 with fixed-bp windows: the gated plans run the LEAN variants, reported as gate = 1;
       SFS2D_LEAN=0 keeps the gated ones)            <F, 2 | 3, 1, 1> without LEAN     fst_gate_nolean, fst_mask_gate_nolean
    otherwise:                       <F, 0, 1, 0>  counts, no Fst (sliced: also k_fst_win's Fst)  nofst, fst_prep (sliced), sliding
                                     <1, 1, 1, 0>  fused counts, Fst from k_prep's sums           fst_prep (fused)
                                     <0, 1, 1, 0>  supplied background, Fst from k_prep's sums    bgsup_norm
                                     <F, 0, 0, 0>  bins plan, no Fst in the scan's arguments      bins_pos, bins_vt (sliced)
                                     <1, 1, 0, 0>  fused bins plan, Fst from k_prep's sums        bins_vt (fused)
                                     <0, 1, 0, 0>  bins plan, supplied background, Fst            bgsup_bins
  k_scan_gw<false, FST, CNT, TRI>   <0|1, 1, 1> 50 x 50 folded counts; <0|1, 1, 0> 100 x 75; <0|1, 0, 0> bins plans
  k_scan_g<false, FST, CNT>         <0|1, 1>, <0|1, 0>                                            (SFS2D_GW=0)
  k_scan_extra<false, CNT>          <1>, <0>: prev_extra plans (the plan's P16 and CNT are the helper's)

Data: synth_genome(3, [6000, 2500, 700], n1p, n2p, seed, n_ann=3); chromosome 0 spans ~335 kb, so a 65,536-bp
scan has 10 windows (6 + 3 + 1) of up to ~1,200 SNPs.  The last test holds a 2D bin of one window with 66,000
SNPs, the case 32-bit bins exist for, on uploaded data with duplicate positions (wrapped data is strictly
increasing by contract)."""
import numpy as np
import pytest

import wide_util as U
from oracle import sfs_oracle as O

pytestmark = pytest.mark.gpu

LENGTHS = [6000, 2500, 700]
W1, W2 = 65536, 131072
VT = "intron_variant"
_DATA, _BG = {}, {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE", "SFS2D_WGS", "SFS2D_LNL",
              "SFS2D_LEAN"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------- data

def genome(name, n1p=25, n2p=25):
    """plain: the synthetic genome; over: five over-called SNPs written into it (test_scan_variants'
    _overcalled_genome words, keys inside the grid, one folding to the excluded last bin); lownc: Fst's edge SNPs
    of test_scan_variants._fst_edge_chrom(True), SNPs with fewer than 2 called alleles among them, over every
    second of chromosome 0's first 1,200 SNPs."""
    key = (name, n1p, n2p)
    if key in _DATA:
        return _DATA[key]
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_genome
    p = synth_genome(3, LENGTHS, n1p, n2p, seed=1000 + 7 * n1p + n2p, n_ann=3)
    counts = p.counts.copy()
    if name == "over":
        assert (n1p, n2p) == (25, 25)
        pc = lambda r1, a1, r2, a2: int(pack_counts(np.array([r1]), np.array([a1]), np.array([r2]), np.array([a2]))[0])
        counts[5] = pc(50, 26, 50, 25)
        counts[777] = pc(40, 20, 30, 10)
        counts[3000] = pc(30, 45, 20, 40)
        counts[6100] = pc(49, 3, 50, 1)
        counts[8600] = pc(10, 50, 12, 45)
    elif name == "lownc":
        assert (n1p, n2p) == (25, 25)
        from test_scan_variants import _fst_edge_chrom
        counts[1:1201:2] = _fst_edge_chrom(True).counts[1:1201:2]
    else:
        assert name == "plain"
    _DATA[key] = PackedSNPs(counts, p.pos, p.chrom_off, list(p.chrom_names), p.ann_id, list(p.ann_names), p.pop1, p.pop2)
    return _DATA[key]


def supplied_bg(p, ocfg, kind):
    """Chromosome 0's background under ocfg: its integer table (kind "int"), or normalised ("norm")."""
    key = (id(p), ocfg.n1p, ocfg.n2p, ocfg.variant_type, ocfg.fold, kind)
    if key not in _BG:
        b2, b1a, b1b = O.chrom_backgrounds(p.subset_chroms([0]), ocfg)[0]
        if kind == "norm":
            b2, b1a, b1b = O.normalize(b2.ravel()).reshape(b2.shape), O.normalize(b1a), O.normalize(b1b)
        _BG[key] = (b2, b1a, b1b)
    return _BG[key]


# W_CASES: id -> (data, ScanConfig keywords, environment, supplied background kind, (fst, cnt, gate) of a fused
# plan, (fst, cnt, gate) of a sliced plan or a plan with a supplied background)
POSF = dict(start_position=20000, end_position=250000)
W_CASES = {
    "nofst": ("plain", {}, {}, None, (0, 1, 0), (0, 1, 0)),
    "fst_gate": ("plain", dict(fst=True), {}, None, (2, 1, 1), (2, 1, 1)),
    "fst_unfold": ("plain", dict(fst=True, fold=False), {}, None, (2, 1, 0), (2, 1, 0)),
    "fst_over": ("over", dict(fst=True), {}, None, (2, 1, 0), (2, 1, 0)),
    "fst_mask_gate": ("lownc", dict(fst=True), {}, None, (3, 1, 1), (3, 1, 1)),
    "fst_mask_nogate": ("lownc", dict(fst=True, fold=False), {}, None, (3, 1, 0), (3, 1, 0)),
    "fst_gate_nolean": ("plain", dict(fst=True), {"SFS2D_LEAN": "0"}, None, (2, 1, 1), (2, 1, 1)),
    "fst_mask_gate_nolean": ("lownc", dict(fst=True), {"SFS2D_LEAN": "0"}, None, (3, 1, 1), (3, 1, 1)),
    "fst_prep": ("plain", dict(fst=True), {"SFS2D_FST_SCAN": "0"}, None, (1, 1, 0), (0, 1, 0)),
    "bins_vt": ("plain", dict(fst=True, vt=VT), {}, None, (1, 0, 0), (0, 0, 0)),
    "bins_pos": ("plain", dict(POSF), {}, None, (0, 0, 0), (0, 0, 0)),
    "wgs1": ("plain", dict(fst=True, scan_wgs_per_cu=1), {}, None, (2, 1, 1), (2, 1, 1)),
    "bgsup_int": ("plain", dict(fst=True), {}, "int", None, (2, 1, 1)),
    "bgsup_norm": ("plain", dict(fst=True), {"SFS2D_FST_SCAN": "0"}, "norm", None, (1, 1, 0)),
    "bgsup_bins": ("plain", dict(fst=True, vt=VT), {}, "int", None, (1, 0, 0)),
}
# (grid, window, fused, case): 25 x 25 takes every case fused and sliced; 18 x 14 and the 131,072-bp window the
# cases that do not need the 25 x 25 fixtures
W_PARAMS = ([(25, 25, W1, f, c) for c in W_CASES for f in ((1, 0) if W_CASES[c][4] else (0,))]
            + [(18, 14, W1, f, c) for c in ("nofst", "fst_gate", "fst_unfold", "fst_prep", "bins_vt", "bins_pos")
               for f in (1, 0)]
            + [(18, 14, W1, 0, "bgsup_norm"), (25, 25, W2, 1, "fst_gate"), (25, 25, W2, 0, "nofst"),
               (18, 14, W2, 0, "fst_gate"), (18, 14, W2, 1, "bins_vt")])


def scan_cfg(p, n1p, n2p, window, vt=None, bg=None, **kw):
    from sfs2d import _lib as L
    from sfs2d.engine import ScanConfig
    return ScanConfig(n1p=n1p, n2p=n2p, window=window, ann_want=-1 if vt is None else p.ann_names.index(vt),
                      bg_mode=L.BG_SUPPLIED if bg else L.BG_PER_CHROM, **kw)


def oracle_cfg(n1p, n2p, kw):
    return O.Cfg(n1p, n2p, kw.get("vt"), kw.get("fold", True), kw.get("start_position"), kw.get("end_position"))


def w_case(n1p, n2p, window, case):
    """(data, ScanConfig, oracle Cfg, supplied background or None, windows, reference key, bg_of) of a W_CASES row."""
    name, kw, _, bgk, _, _ = W_CASES[case]
    p = genome(name, n1p, n2p)
    ocfg = oracle_cfg(n1p, n2p, kw)
    bg = supplied_bg(p, ocfg, bgk) if bgk else None
    cfg = scan_cfg(p, n1p, n2p, window, bg=bgk, **kw)
    if bg is None:
        bkey = ("bgs", name, n1p, n2p, kw.get("vt"), kw.get("fold", True), kw.get("start_position"))
        if bkey not in _BG:
            _BG[bkey] = O.chrom_backgrounds(p, ocfg)
        bgs = _BG[bkey]
        bg_of = lambda c: bgs[c]
    else:
        bg_of = lambda c: bg
    key = ("w", name, n1p, n2p, window, kw.get("vt"), kw.get("fold", True), kw.get("start_position"), bgk)
    return p, cfg, ocfg, bg, O.bp_windows(p, window), key, bg_of


def both(p, cfg, want, bg=None):
    """The plan on wrapped data (its variant: `want` with p16 = 0) and on uploaded data (p16 = 1), the two
    tables' integers and flags identical; returns the wrapped run's (records, Fst)."""
    from sfs2d.engine import Engine
    eng = Engine.get(0)
    d, keep = U.wrapped(eng, p, ann=cfg.ann_want >= 0)
    try:
        rw, fw, vw = U.run_plan(d, cfg, bg)
    finally:
        d.close()
        del keep
    assert vw == dict(want, p16=0), (vw, want)
    dev = eng.upload(p)
    try:
        ru, fu, vu = U.run_plan(dev, cfg, bg)
    finally:
        dev.close()
    assert vu == dict(want, p16=1), (vu, want)
    U.same_ints(rw, ru)
    return rw, fw


@pytest.mark.parametrize("n1p,n2p,window,fused,case", W_PARAMS,
                         ids=[f"{a}x{b}-{w}-{'fused' if f else 'sliced'}-{c}" for a, b, w, f, c in W_PARAMS])
def test_scan_w_wide(monkeypatch, n1p, n2p, window, fused, case):
    _, _, env, bgk, vf, vs = W_CASES[case]
    monkeypatch.setenv("SFS2D_FUSED", "1" if fused else "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, cfg, ocfg, bg, wins, key, bg_of = w_case(n1p, n2p, window, case)
    fst, cnt, gate = vf if fused else vs
    recs, f = both(p, cfg, dict(fused=0 if bgk else fused, fst=fst, cnt=cnt, gate=gate, tri=-1), bg)
    U.check_against_oracle(recs, f, p, wins, ocfg, bg_of, key=key)


# ------------------------------------------------------------------------------------------- Q9 helper

@pytest.mark.parametrize("vt", [None, VT], ids=["counts", "bins"])
def test_scan_extra_wide(monkeypatch, vt):
    """k_scan_extra<false, CNT>: the record after the slots is the window before the last one evaluated against
    the last window's chromosome background, as combined_scan's final block (fake_records.bp_records builds it
    from the oracle)."""
    import fake_records as FR
    import golden_util as gu
    from sfs2d import _lib as L
    monkeypatch.setenv("SFS2D_FUSED", "1")
    p = genome("plain")
    kw = dict(vt=vt)
    ocfg = oracle_cfg(25, 25, kw)
    cfg = scan_cfg(p, 25, 25, W1, prev_extra=True, **kw)
    bgs = O.chrom_backgrounds(p, ocfg)
    recs, _ = both(p, cfg, dict(fused=1, fst=0, cnt=0 if vt else 1, gate=0, tri=-1))
    U.check_against_oracle(recs, None, p, O.bp_windows(p, W1), ocfg, lambda c: bgs[c])
    want = FR.bp_records(p, W1, ocfg, lambda c: bgs[c], prev_extra=True)
    assert len(recs) == len(want)
    x, y = recs[-1], want[-1]
    assert int(x["flags"]) & L.W_EXTRA and not int(x["flags"]) & L.W_EMPTY
    for k in ("chrom", "begin", "end", "snp_count", "n2", "n2_all", "n1a", "n1b"):
        assert int(x[k]) == int(y[k]), (k, int(x[k]), int(y[k]))
    for k in ("t2d", "t1d_p1", "t1d_p2"):
        assert float(y[k]) != 0.0 and gu.close(float(x[k]), float(y[k])), (k, float(x[k]), float(y[k]))


# ------------------------------------------------------------------------------------------- large grids

G_PARAMS = ([(50, 50, vt, fst, gw) for vt in (None, VT) for fst in (False, True) for gw in (1, 0)]
            + [(100, 75, None, False, 1), (100, 75, None, True, 1), (100, 75, None, True, 0)])


@pytest.mark.parametrize("n1p,n2p,vt,fst,gw", G_PARAMS,
                         ids=[f"{a}x{b}-{'bins' if v else 'counts'}-{'fst' if f else 'nofst'}-gw{g}" for a, b, v, f, g in G_PARAMS])
def test_large_grids_wide(monkeypatch, n1p, n2p, vt, fst, gw):
    """k_scan_gw<false, FST, CNT, TRI> (SFS2D_GW=1) and k_scan_g<false, FST, CNT> (SFS2D_GW=0): 50 x 50 folded
    counts keep the reachable triangle (TRI), 100 x 75 and bins plans the full grid."""
    monkeypatch.setenv("SFS2D_GW", str(gw))
    p = genome("plain", n1p, n2p)
    kw = dict(vt=vt)
    ocfg = oracle_cfg(n1p, n2p, kw)
    cfg = scan_cfg(p, n1p, n2p, W1, fst=fst, **kw)
    bkey = ("bgs", "plain", n1p, n2p, vt, True, None)
    if bkey not in _BG:
        _BG[bkey] = O.chrom_backgrounds(p, ocfg)
    bgs = _BG[bkey]
    cnt = 0 if vt else 1
    want = dict(fused=-1, fst=int(fst), cnt=cnt, gate=-1, tri=(1 if cnt and n1p == n2p else 0) if gw else -1)
    recs, f = both(p, cfg, want)
    U.check_against_oracle(recs, f, p, O.bp_windows(p, W1), ocfg, lambda c: bgs[c],
                           key=("w", "plain", n1p, n2p, W1, vt, True, None, None))


# ------------------------------------------------------------------------------------------- sliding

@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "sliced"])
@pytest.mark.parametrize("fst_scan", [True, False], ids=["fst_in_scan", "fst_win"])
def test_sliding_wide(monkeypatch, fused, fst_scan):
    """A sliding plan on wrapped data (step = window / 4): the bound on a window's SNPs needs host positions, so
    32-bit bins; against windows built from the definition (wide_util.sliding_slots).  SFS2D_FST_SCAN=0: Fst by
    k_fst_win over the sliding slots, FST = 0 in the scan's arguments."""
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    if not fst_scan:
        monkeypatch.setenv("SFS2D_FST_SCAN", "0")
    p = genome("plain")
    ocfg = O.Cfg(25, 25)
    cfg = scan_cfg(p, 25, 25, W1, fst=True, step=W1 // 4)
    bkey = ("bgs", "plain", 25, 25, None, True, None)
    if bkey not in _BG:
        _BG[bkey] = O.chrom_backgrounds(p, ocfg)
    bgs = _BG[bkey]
    slots = U.sliding_slots(p, W1, W1 // 4)
    wins = [s for s in slots if s[2] < s[3]]
    v = (2, 1, 1) if fst_scan else (0, 1, 0)
    recs, f = both(p, cfg, dict(fused=fused, fst=v[0], cnt=v[1], gate=v[2], tri=-1))
    assert len(recs) == len(slots) and [int(r["wid"]) for r in recs] == [s[1] for s in slots]
    U.check_against_oracle(recs, f, p, wins, ocfg, lambda c: bgs[c], key=("slide", W1))


# ------------------------------------------------------------------------------------------- attached

@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "sliced"])
def test_attached_wide(monkeypatch, fused):
    """A wrapped 16,384-bp base (16-bit bins: unique positions bound its windows) with an attached 131,072-bp
    plan (32-bit bins) and an attached 300-SNP plan (16-bit), Fst on: each plan's own variant, each table
    against the oracle."""
    from sfs2d import _lib as L
    from sfs2d.engine import Engine
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    p = genome("plain")
    ocfg = O.Cfg(25, 25)
    bkey = ("bgs", "plain", 25, 25, None, True, None)
    if bkey not in _BG:
        _BG[bkey] = O.chrom_backgrounds(p, ocfg)
    bgs = _BG[bkey]
    eng = Engine.get(0)
    d, keep = U.wrapped(eng, p)
    base = None
    try:
        base = eng.plan(d, scan_cfg(p, 25, 25, 16384, fst=True))
        a_bp = base.attach(scan_cfg(p, 25, 25, W2, fst=True))
        a_snp = base.attach(scan_cfg(p, 25, 25, 300, fst=True, window_mode=L.WINDOW_SNPS))
        with pytest.raises(L.Sfs2dError):
            a_bp.scan_variant()   # nothing has run
        base.run()
        base.check()
        out = [(q.read(), q.read_fst(), q.scan_variant()) for q in (base, a_bp, a_snp)]
    finally:
        if base is not None:
            base.close()
        d.close()
        del keep
    for (_, _, v), p16 in zip(out, (1, 0, 1)):
        assert v == dict(p16=p16, fused=fused, fst=2, cnt=1, gate=1, tri=-1), v
    wins = [O.bp_windows(p, 16384), O.bp_windows(p, W2), O.snp_windows(p, 300)[0]]
    keys = [("w", "plain", 25, 25, 16384, None, True, None, None), ("w", "plain", 25, 25, W2, None, True, None, None),
            ("snp", 300)]
    for (recs, f, _), w, k in zip(out, wins, keys):
        U.check_against_oracle(recs, f, p, w, ocfg, lambda c: bgs[c], key=k)


# ------------------------------------------------------------------------------------------- a bin past 65,535

BIG, BIG_WS, BIG_SNPS = 66000, 40000, 70000


def big_bin_genome():
    """Chromosome 0: 300 mixed SNPs (positions 1 .. ~17 kb), 66,000 SNPs of one in-grid counts word at 4 per
    position (20,001 .. 36,500), then 4,000 mixed SNPs from 38,000 on; chromosome 1: 3,000 ordinary SNPs, which
    give the per-chromosome background other windows, so that T is not 0.  40,000-bp windows: the first holds
    the 300, the 66,000 and the mixed SNPs up to 40,000; as SNP-count windows of 70,000 the chromosome is one
    window (300 + 66,000 + 3,700: the trailing run is 4,000 rather than 300 so that such a window exists)."""
    if "big" in _DATA:
        return _DATA["big"]
    from sfs2d.pack import PackedSNPs, pack_counts
    from sfs2d.synth import synth_chrom
    rng = np.random.Generator(np.random.PCG64(66))
    pos0, r1, a1, r2, a2 = synth_chrom(rng, 4300, 25, 25)
    mixed = pack_counts(r1, a1, r2, a2)
    word = int(pack_counts(np.array([47]), np.array([3]), np.array([30]), np.array([20]))[0])
    pos1, s1, b1, s2, b2 = synth_chrom(rng, 3000, 25, 25)
    counts = np.concatenate([mixed[:300], np.full(BIG, word, np.uint32), mixed[300:], pack_counts(s1, b1, s2, b2)])
    pos = np.concatenate([pos0[:300], 20001 + np.arange(BIG) // 4, 38000 + (pos0[300:] - pos0[300]), pos1])
    assert pos0[299] < 20001
    n0 = 4300 + BIG
    _DATA["big"] = PackedSNPs(counts, pos.astype(np.uint32), np.array([0, n0, n0 + 3000], np.int64), ["chr0000", "chr0001"],
                              np.zeros(n0 + 3000, np.uint16), ["intergenic_region"], "p1", "p2")
    return _DATA["big"]


def big_bin_ref(snps):
    p = big_bin_genome()
    ocfg = O.Cfg(25, 25)
    if "big_bgs" not in _BG:
        _BG["big_bgs"] = O.chrom_backgrounds(p, ocfg)
    bgs = _BG["big_bgs"]
    wins = O.snp_windows(p, BIG_SNPS)[0] if snps else O.bp_windows(p, BIG_WS)
    return p, ocfg, wins, U.oracle_ref(p, wins, ocfg, lambda c: bgs[c], key=("big", snps))


BIG_PARAMS = [(False, 1, True), (False, 0, True), (True, 1, True), (False, 1, False), (False, 0, False), (True, 0, False)]


@pytest.mark.parametrize("snps,fused,fst", BIG_PARAMS,
                         ids=[f"{'snps' if s else 'bp'}-{'fused' if f else 'sliced'}-{'fst' if t else 'nofst'}" for s, f, t in BIG_PARAMS])
def test_bin_of_66000_snps(monkeypatch, snps, fused, fst):
    """One 2D bin of one window holds 66,000 SNPs (a 16-bit bin would wrap): uploaded data with 4 SNPs per
    position, so plan_create finds the longest window from the host positions.  A window of >= 65,535 SNPs is
    re-evaluated by eval_exact, its end read from the slot record: without Fst in the scan the flush used to
    clear that record first (the nofst cases).  T under the `wide` rule of test_null_gpu._check
    (wide_util.wide_scale), Fst summed in the scan within 1e-12 + 1e-10 |x|."""
    from sfs2d import _lib as L
    from sfs2d.engine import Engine
    monkeypatch.setenv("SFS2D_FUSED", str(fused))
    p, ocfg, wins, ref = big_bin_ref(snps)
    cfg = scan_cfg(p, 25, 25, BIG_SNPS if snps else BIG_WS, fst=fst, window_mode=L.WINDOW_SNPS if snps else L.WINDOW_BP)
    dev = Engine.get(0).upload(p)
    try:
        recs, f, v = U.run_plan(dev, cfg)
    finally:
        dev.close()
    assert v == dict(p16=0, fused=fused, fst=2 if fst else 0, cnt=1, gate=1 if fst else 0, tri=-1), v
    U.check_records(recs, f, ref, wide=True)
