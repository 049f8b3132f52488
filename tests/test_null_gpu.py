"""The bootstrap null on the device (kernel k_null, sfs2d_plan_null_run) against its
host twin: sfs2d.null.resample (the same draws from synth._philox) evaluated by oracle.window_records.

Record parity compares EVERY record of every task: integer fields exact, validity (n > 0 and no BG-zero
flag) and the BG-zero flags identical, T within golden_util.close (1e-10 relative, inf / NaN by identity)
wherever the oracle has a value.  The genome's chromosomes hold 3,000 / 5 / 1,200 SNPs: pool 1 is tiny, so
its windows are mostly repeats; m = 1, 2 (one Philox call), 63, 64, 65 (a wave's pairs: 32, 32, 33 lanes),
129 (65 pairs: a second round), 700 (350 pairs > 4 x 64: the draws kept in registers run out and the rest
are drawn again in the take pass).

T = 2 (S - N ln N) is a difference of sums of ~N ln N (thousands here), so any evaluation order -- scipy's
gammaln differences in the oracle as much as the kernel's -- carries ~1e-12 of absolute rounding error.  The
project's fixtures keep oracle T's out of (0, 1e-2) for that reason (test_filtered_plans._no_cancelled_t);
these tasks are fixed and 700 draws from a 7 x 5 grid do give T1D ~ 3e-3, so such values are compared too,
with the relative 1e-10 taken of max(|T|, 1e-2): the absolute error the project's bound allows at its own
threshold (1e-12), never more."""
import csv
import ctypes as C
import os

import numpy as np
import pytest

import golden_util as gu
import null_util as U
from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import null as N

pytestmark = pytest.mark.gpu

LENGTHS = [3000, 5, 1200]
MS = [1, 2, 63, 64, 65, 129, 700]
R, SEED = 37, 5
W = 20000
VT = "intron_variant"
INTS = U.INTS
T_FLOOR = U.T_FLOOR   # see the module docstring
_DATA, _TWIN = {}, {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE"):
        monkeypatch.delenv(k, raising=False)


def _genome(n1p, n2p):
    from sfs2d.synth import synth_genome
    if (n1p, n2p) not in _DATA:
        _DATA[(n1p, n2p)] = synth_genome(3, LENGTHS, n1p, n2p, seed=7, n_ann=3)
    return _DATA[(n1p, n2p)]


def _tasks(pools):
    return [(c, m) for c in pools for m in MS]


def _twin(n1p, n2p, fold=True, vt=None, start=None, end=None, bg=None, pools=(0, 2)):
    """The expected records (computed once per configuration, shared by the plan flavours).  bg: None = each
    pool's own chromosome; "int" / "norm" = chromosome 0's background, integer or normalised."""
    key = (n1p, n2p, fold, vt, start, end, bg, pools)
    if key not in _TWIN:
        p = _genome(n1p, n2p)
        cfg = O.Cfg(n1p, n2p, vt, fold, start, end)
        bgs = O.chrom_backgrounds(p, cfg)
        if bg == "norm":
            one = tuple(O.normalize(np.asarray(x).ravel()).reshape(np.asarray(x).shape) for x in bgs[0])
        elif bg == "int":
            one = bgs[0]
        bg_of = (lambda c: bgs[c]) if bg is None else (lambda c: one)
        recs, _, _ = U.null_twin(p, _tasks(pools), R, SEED, cfg, bg_of)
        _TWIN[key] = (recs, None if bg is None else one)
    return _TWIN[key]


_check = U.check


def _engine():
    from sfs2d.engine import Engine
    return Engine.get(0)


def _cfg(n1p, n2p, **kw):
    from sfs2d.engine import ScanConfig
    kw.setdefault("window_mode", L.WINDOW_BP)
    kw.setdefault("window", W)
    return ScanConfig(n1p=n1p, n2p=n2p, **kw)


def _null_records(p, cfg, tasks, bg=None, kernel=None, seed=SEED, reps=R):
    eng = _engine()
    dev = eng.upload(p)
    try:
        pl = eng.plan(dev, cfg)
        try:
            if bg is not None:
                pl.set_background(*bg)
            pl.run()
            pl.check()
            if kernel is not None:
                assert pl.scan_kernel() == kernel
            pl.null_run(tasks, reps, seed)
            return pl.null_read()
        finally:
            pl.close()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------- record parity

# every way a plan leaves (or does not leave) its per-chromosome tables in global memory
FLAVOURS = {"sliced": ({"SFS2D_FUSED": "0"}, "k_scan_w"), "fused": ({"SFS2D_FUSED": "1"}, "k_scan_w"),
            "gw": ({"SFS2D_GW": "1"}, "k_scan_gw"), "g": ({"SFS2D_GW": "0"}, "k_scan_g")}


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
@pytest.mark.parametrize("size,flavour", [((3, 2), "sliced"), ((3, 2), "fused"), ((18, 14), "sliced"), ((18, 14), "fused"),
                                          ((100, 75), "gw"), ((100, 75), "g")])
def test_record_parity_grids(monkeypatch, size, flavour, fold):
    env, kernel = FLAVOURS[flavour]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n1p, n2p = size
    want, _ = _twin(n1p, n2p, fold)
    got = _null_records(_genome(n1p, n2p), _cfg(n1p, n2p, fold=fold, bg_mode=L.BG_PER_CHROM), _tasks((0, 2)), kernel=kernel)
    assert _check(got, want) > len(want)   # (most records have all three statistics)


@pytest.mark.parametrize("flavour", ["sliced", "fused"])
def test_record_parity_variant_type(monkeypatch, flavour):
    """A bins plan: a drawn SNP that the variant_type filter excludes stays out of the spectra, counts
    toward m and not toward snp_count."""
    monkeypatch.setenv("SFS2D_FUSED", FLAVOURS[flavour][0]["SFS2D_FUSED"])
    p = _genome(18, 14)
    want, _ = _twin(18, 14, vt=VT)
    got = _null_records(p, _cfg(18, 14, bg_mode=L.BG_PER_CHROM, ann_want=p.ann_names.index(VT)), _tasks((0, 2)))
    _check(got, want)
    big = got[got["end"] == 700]
    assert np.all(big["snp_count"] < 700) and np.all(big["snp_count"] > 100) and np.all(big["n2_all"] <= big["snp_count"])


def test_record_parity_position_filter():
    p = _genome(18, 14)
    start, end = int(p.pos[700]), int(p.pos[2300])     # inside chromosome 0; chromosome 2's positions overlap it
    want, _ = _twin(18, 14, start=start, end=end)
    got = _null_records(p, _cfg(18, 14, bg_mode=L.BG_PER_CHROM, start_position=start, end_position=end), _tasks((0, 2)))
    _check(got, want)
    big = got[got["end"] == 700]
    assert np.all(big["snp_count"] == 700) and np.all(big["n2_all"] < 700) and np.all(big["n2_all"] > 100)


@pytest.mark.parametrize("kind", ["int", "norm"])
def test_record_parity_supplied_background(kind):
    """One supplied table for every pool -- chromosome 0's background as scan_chooseChr passes it (integer
    counts, fixed-bp windows) and as scan_chooseChr_bySNPs does (normalised, SNP-count windows) -- with the
    tiny pool 1 and pool -1, all 4,205 SNPs.  Windows that touch a bin the table lacks have T = +inf."""
    p = _genome(18, 14)
    want, bg = _twin(18, 14, bg=kind, pools=(1, -1))
    cfg = _cfg(18, 14, bg_mode=L.BG_SUPPLIED) if kind == "int" else _cfg(18, 14, bg_mode=L.BG_SUPPLIED,
                                                                         window_mode=L.WINDOW_SNPS, window=50)
    got = _null_records(p, cfg, _tasks((1, -1)), bg=bg)
    _check(got, want)
    assert np.all(got["chrom"][: len(MS) * R] == 1) and np.all(got["chrom"][len(MS) * R:] == 0xFFFFFFFF)


def test_record_parity_sliding_plan():
    want, _ = _twin(18, 14)
    got = _null_records(_genome(18, 14), _cfg(18, 14, bg_mode=L.BG_PER_CHROM, step=W // 4, fst=True), _tasks((0, 2)))
    _check(got, want)


def test_record_parity_wide_bins():
    """m = 65,535 still packs two 2D bins per LDS word, m = 65,536 takes 32-bit bins (a bin could wrap)."""
    p = _genome(3, 2)
    cfg = O.Cfg(3, 2)
    bgs = O.chrom_backgrounds(p, cfg)
    for m in (65535, 65536):
        want, _, _ = U.null_twin(p, [(2, m)], 2, SEED, cfg, lambda c: bgs[c])
        _check(_null_records(p, _cfg(3, 2, bg_mode=L.BG_PER_CHROM), [(2, m)], reps=2), want, wide=True)


# ------------------------------------------------------------------------------------------- independence

def test_records_depend_on_the_task_alone(monkeypatch):
    import torch
    p = _genome(18, 14)
    cfg = _cfg(18, 14, bg_mode=L.BG_PER_CHROM)
    tasks = _tasks((0, 2))
    eng = _engine()
    dev = eng.upload(p)
    try:
        pl = eng.plan(dev, cfg)
        try:
            pl.run()
            pl.check()
            pl.null_run(tasks, R, SEED)
            a = pl.null_read()
            pl.null_run(tasks[::-1], R, SEED)
            b = pl.null_read()
            pl.null_run(tasks[:5], R, SEED)
            c1 = pl.null_read()
            pl.null_run(tasks[5:], R, SEED)
            c2 = pl.null_read()
            pl.null_run(tasks, R, SEED + 1)
            d = pl.null_read()
            pl.null_run(tasks, 5, SEED)           # fewer replicates: the same first five
            e = pl.null_read()
            # Plan.null_run's own split (one call writes at most MAX_CALL_RECORDS records): 3 tasks per call
            # here, to the host and into a caller's device buffer
            monkeypatch.setattr(N, "MAX_CALL_RECORDS", 3 * R)
            pl.null_run(tasks, R, SEED)
            f = pl.null_read()
            buf = torch.zeros(len(tasks) * R * 64, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            pl.null_run(tasks, R, SEED, out_dev_ptr=buf.data_ptr())
            pl.check()                            # (synchronises the engine's stream)
            g = buf.cpu().numpy().view(L.WINDOW_DTYPE)
            with pytest.raises(ValueError):
                pl.null_read()                    # the records went to the caller's buffer
        finally:
            pl.close()
    finally:
        dev.close()
    by_task = lambda x: x.reshape(-1, R)
    assert by_task(a).tobytes() == by_task(b)[::-1].tobytes()
    assert a.tobytes() == np.concatenate([c1, c2]).tobytes()
    assert e.tobytes() == by_task(a)[:, :5].tobytes()
    assert f.tobytes() == a.tobytes() and g.tobytes() == a.tobytes()
    differ = by_task(a)["n2_all"] != by_task(d)["n2_all"]
    assert np.all(differ[np.array([m for _, m in tasks]) >= 63].any(axis=1))   # another seed: other draws
    assert np.array_equal(a[INTS[0]], d[INTS[0]]) and np.array_equal(a["end"], d["end"])


# ------------------------------------------------------------------------------------------- plan untouched

@pytest.mark.parametrize("flavour", ["sliced", "fused", "gw", "sliding", "supplied"])
def test_null_run_leaves_the_plan_as_it_found_it(monkeypatch, flavour):
    """run, read records and Fst, null_run (twice: the second finds the tables the first built), run again
    twice (both buffer parities): records and Fst byte-equal."""
    size = (100, 75) if flavour == "gw" else (18, 14)
    if flavour in FLAVOURS:
        for k, v in FLAVOURS[flavour][0].items():
            monkeypatch.setenv(k, v)
    p = _genome(*size)
    kw = dict(bg_mode=L.BG_SUPPLIED if flavour == "supplied" else L.BG_PER_CHROM, fst=True)
    if flavour == "sliding":
        kw["step"] = W // 4
    eng = _engine()
    dev = eng.upload(p)
    try:
        pl = eng.plan(dev, _cfg(*size, **kw))
        try:
            if flavour == "supplied":
                pl.set_background(*O.chrom_backgrounds(p, O.Cfg(*size))[0])
            pl.run()
            pl.check()
            recs, fst = pl.read(), pl.read_fst()
            assert len(recs) > 10 and np.isfinite(fst).any()
            pool = 1 if flavour == "supplied" else 2
            for _ in range(2):
                pl.null_run([(pool, 64), (0, 5)], 9, SEED)
                first = pl.null_read()
            for _ in range(2):
                pl.run()
                pl.check()
                assert pl.read().tobytes() == recs.tobytes() and pl.read_fst().tobytes() == fst.tobytes()
            pl.null_run([(pool, 64), (0, 5)], 9, SEED)
            assert pl.null_read().tobytes() == first.tobytes()      # and the null of the new run is the same
        finally:
            pl.close()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------- refusals

def test_refusals():
    from sfs2d.synth import synth_genome
    p = synth_genome(3, [400, 0, 300], 18, 14, seed=3)               # chromosome 1 is empty
    eng = _engine()
    dev = eng.upload(p)

    def refused(pl, tasks, reps=3):
        with pytest.raises(L.Sfs2dError) as ei:
            pl.null_run(tasks, reps, SEED)
        assert ei.value.code == L.E_ARG and len(str(ei.value)) > len("sfs2d error -1: ")
        return str(ei.value)
    try:
        pl = eng.plan(dev, _cfg(18, 14, bg_mode=L.BG_PER_CHROM))
        sup = eng.plan(dev, _cfg(18, 14, bg_mode=L.BG_SUPPLIED))
        try:
            att = pl.attach(_cfg(18, 14, bg_mode=L.BG_PER_CHROM, window=2 * W))
            assert "run" in refused(pl, [(0, 5)])                    # a plan that has not run
            pl.run()
            pl.check()
            assert "attached" in refused(att, [(0, 5)])              # an attached plan: use its base
            assert "out of range" in refused(pl, [(0, 5), (3, 5)])   # pool out of range
            assert "out of range" in refused(pl, [(-2, 5)])
            assert "-1" in refused(pl, [(-1, 5)])                    # all SNPs on a per-chromosome plan
            assert "empty" in refused(pl, [(1, 5)])                  # an empty pool
            assert "m must" in refused(pl, [(0, 0)])                 # m < 1
            assert "m must" in refused(pl, [(0, -3)])
            assert "replicates" in refused(pl, [(0, 5)], reps=0)     # replicates < 1
            sup.set_background(*O.chrom_backgrounds(p, O.Cfg(18, 14))[0])
            assert "run" in refused(sup, [(-1, 5)])
            sup.run()
            assert "empty" in refused(sup, [(1, 5)])
            sup.null_run([(-1, 5)], 3, SEED)                         # fine on a supplied-background plan
            assert len(sup.null_read()) == 3
            # capacity: null_read reports the count and refuses a smaller buffer
            pl.null_run([(0, 5), (2, 6)], 3, SEED)
            n = C.c_int64()
            buf = np.zeros(5, L.WINDOW_DTYPE)
            assert eng.lib.sfs2d_plan_null_read(pl.h, L.ptr(buf), 5, C.byref(n)) == L.E_CAP and n.value == 6
            assert len(pl.null_read()) == 6
        finally:
            pl.close()
            sup.close()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------- end to end

def _slots(p, w, s):
    out = []
    for c in range(p.nchrom):
        lo, hi = int(p.chrom_off[c]), int(p.chrom_off[c + 1])
        pos = p.pos[lo:hi].astype(np.int64)
        js = np.arange((int(pos[-1]) - 1) // s + 1, dtype=np.int64)
        b = np.searchsorted(pos, js * s + 1, "left")
        b[0] = 0
        e = np.searchsorted(pos, js * s + w + 1, "left")
        out += [(c, int(j), lo + int(x), lo + int(max(x, y))) for j, x, y in zip(js, b, e)]
    return out


def _expected_p(p, cfg, windows_by_label, rows_by_size, reps, seed):
    """null.pvalues over oracle twins: the observed windows of every requested size from the oracle, one
    null task per (chromosome, default size class) over the union of the sizes."""
    bgs = O.chrom_backgrounds(p, cfg)
    bg_of = lambda c: bgs[c]
    wins = [w for key in rows_by_size for lb, w in windows_by_label[key].items() if lb in rows_by_size[key]]
    obs = U.oracle_records(p, wins, cfg, bg_of, wid_of=lambda w: 0)
    cls = N.size_classes(obs["end"])
    tasks = sorted(set(zip(obs["chrom"].tolist(), cls.tolist())))
    null, _, _ = U.null_twin(p, tasks, reps, seed, cfg, bg_of)
    pv = N.pvalues(obs, null, cls)
    out, k = {}, 0
    for key in rows_by_size:
        for lb in windows_by_label[key]:
            if lb in rows_by_size[key]:
                out[(key, lb)] = {name: (None if np.isnan(pv[name][k]) else float(pv[name][k])) for name in N.P_KEYS}
                k += 1
    assert k == len(obs)
    return out, len(tasks)


def _strip(rows):
    return {lb: {k: v for k, v in r.items() if not k.startswith("p_")} for lb, r in rows.items()}


def test_scan_pvalues_end_to_end():
    import twoDSFS_class as T
    from sfs2d.synth import synth_genome
    p = synth_genome(2, [4000, 4000], 18, 14, seed=21)
    cfg = O.Cfg(18, 14)
    names = p.chrom_names
    obj = T.LikelihoodInference_jointSFS(None, None, pop1=p.pop1, pop2=p.pop2, pop1_size=18, pop2_size=14)
    reps, seed = 49, 3
    # disjoint windows: 2 kb, 8 kb and 40 SNPs from one pass, one null run
    got = obj.scan_pvalues(p, window_sizes=(2000, 8000), snp_window_sizes=(40,), replicates=reps, seed=seed)
    plain = obj.multi_scan(p, (2000, 8000), (40,))
    assert list(got) == list(plain) == [2000, 8000, "40snps"]
    labels = {ws: {f"{names[c]} {s}-{s + ws - 1}": (c, b, e) for c, s, b, e in O.bp_windows(p, ws)} for ws in (2000, 8000)}
    labels["40snps"] = {f"{names[c]} {s}-{ep}": (c, b, e) for c, s, ep, b, e in O.snp_windows(p, 40)[0]}
    want, ntasks = _expected_p(p, cfg, labels, got, reps, seed)
    assert ntasks > 20
    for key in got:
        assert _strip(got[key]) == plain[key] and len(got[key]) > 50
        for lb, row in got[key].items():
            assert list(row)[-6:] == list(N.P_KEYS)
            assert {k: row[k] for k in N.P_KEYS} == want[(key, lb)], (key, lb)
    # sliding windows, step 1 kb
    got = obj.scan_pvalues(p, window_sizes=(2000, 8000), step_size=1000, replicates=reps, seed=seed)
    plain = obj.multi_sliding_scan(p, (2000, 8000), 1000)
    labels = {ws: {f"{names[c]} {j * 1000 + 1}-{j * 1000 + ws}": (c, b, e) for c, j, b, e in _slots(p, ws, 1000) if e > b}
              for ws in (2000, 8000)}
    want, _ = _expected_p(p, cfg, labels, got, reps, seed)
    for key in got:
        assert _strip(got[key]) == plain[key] and list(got[key]) == list(labels[key])
        for lb, row in got[key].items():
            assert {k: row[k] for k in N.P_KEYS} == want[(key, lb)], (key, lb)
    # every p-value is k / (R + 1) with 1 <= k <= R + 1
    ps = np.array([row[k] for rows in got.values() for row in rows.values() for k in N.P_KEYS if row[k] is not None])
    assert np.all(np.abs(ps * (reps + 1) - np.rint(ps * (reps + 1))) < 1e-9) and ps.min() >= 1 / (reps + 1) and ps.max() <= 1.0


def test_scan_pvalues_background_chromosome_and_sizes():
    """One chromosome as background and pool of every window (scan_chooseChr's scan), sizes="exact"."""
    import twoDSFS_class as T
    from sfs2d.synth import synth_genome
    p = synth_genome(2, [1500, 800], 18, 14, seed=22)
    cfg = O.Cfg(18, 14)
    obj = T.LikelihoodInference_jointSFS(None, None, pop1=p.pop1, pop2=p.pop2, pop1_size=18, pop2_size=14)
    got = obj.scan_pvalues(p, window_sizes=(8000,), background_chromosome="chr0001", replicates=29, seed=1, sizes="exact")
    assert list(got) == [8000] and _strip(got[8000]) == obj.scan_chooseChr(p, 8000, "chr0001")
    bg = O.chrom_backgrounds(p, cfg)[1]
    wins = {f"{p.chrom_names[c]} {s}-{s + 7999}": (c, b, e) for c, s, b, e in O.bp_windows(p, 8000)}
    assert list(wins) == list(got[8000])
    obs = U.oracle_records(p, list(wins.values()), cfg, lambda c: bg, wid_of=lambda w: 0)
    tasks = sorted(set((1, int(m)) for m in obs["end"]))
    null, _, _ = U.null_twin(p, tasks, 29, 1, cfg, lambda c: bg)
    pv = N.pvalues(obs, null, obs["end"], pools=np.ones(len(obs), np.int64))
    for k, row in enumerate(got[8000].values()):
        assert {n: row[n] for n in N.P_KEYS} == {n: (None if np.isnan(pv[n][k]) else float(pv[n][k])) for n in N.P_KEYS}
    with pytest.raises(ValueError):
        obj.scan_pvalues(p, window_sizes=(8000, 16000), background_chromosome="chr0001")
    with pytest.raises(ValueError, match="below the largest window"):
        obj.scan_pvalues(p, window_sizes=(8000,), sizes=[10, 20])
    dist = T.LikelihoodInference_jointSFS(None, None, pop1_size=18, pop2_size=14, distributed=True)
    with pytest.raises(NotImplementedError):
        dist.scan_pvalues(p, window_sizes=(8000,))


def test_cli_null_columns(tmp_path):
    """--null-replicates 99 appends the six p_* columns (after FST) to every file; the other columns, and the
    files written without the option, are what multi_scan + write_csv give."""
    import twoDSFS_class as T
    from sfs2d import cli
    from sfs2d.vcf import read_vcf
    vcf, pm = os.path.join(gu.GOLD, "vcf_test.vcf.gz"), os.path.join(gu.GOLD, "popmap_3pop.txt")
    base = [vcf, pm, "--pop1", "uv", "--pop2", "bv", "--pop1-size", "11", "--pop2-size", "11", "--fst",
            "--window", "500000", "--window", "1000000", "--snp-window", "100"]
    plain = cli.main(base + ["--out-prefix", str(tmp_path / "plain")])
    null = cli.main(base + ["--out-prefix", str(tmp_path / "null"), "--null-replicates", "99", "--null-seed", "4"])
    assert [os.path.basename(o) for o in null] == ["null_500kb.csv", "null_1000kb.csv", "null_100snps.csv"]
    # without the option: byte-equal to the files of the scan drivers alone
    p = read_vcf(vcf, pm).to_packed("uv", "bv")
    obj = T.LikelihoodInference_jointSFS(vcf, pm, pop1_size=11, pop2_size=11)
    res = obj.multi_scan(p, [500000, 1000000], [100], fst=True)
    for path, key in zip(plain, (500000, 1000000, "100snps")):
        ref = str(tmp_path / "ref.csv")
        fst = res["fst"][key] if key != "100snps" else obj.window_fst(p, snp_window_size=100)
        cli.write_csv(ref, res[key], {}, fst, None)
        assert open(path, "rb").read() == open(ref, "rb").read()
    seen = 0
    for a, b in zip(plain, null):
        with open(a, newline="") as fa, open(b, newline="") as fb:
            ra, rb = list(csv.DictReader(fa)), list(csv.DictReader(fb))
        assert list(ra[0]) == T.col_names + ["FST"] and list(rb[0]) == T.col_names + ["FST"] + cli.P_COLS
        assert len(ra) == len(rb) > 0
        for x, y in zip(ra, rb):
            assert x == {k: y[k] for k in x}
            for c in cli.P_COLS:
                assert y[c] == "" or 1 / 100 <= float(y[c]) <= 1.0
                seen += y[c] != ""
            assert (y["p_T2D"] == "") == (y["T2D"] == "")
    assert seen > 100
