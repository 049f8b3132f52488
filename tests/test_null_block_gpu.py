"""The block bootstrap null on the device (kernel k_null_blk, sfs2d_plan_null_run_blocks; DESIGN.md section 14,
"blocks") against its host twin: sfs2d.null.resample(..., block=b) -- the same block starts from
synth._philox, runs of consecutive SNPs of the circular pool -- evaluated by oracle.window_records.

Fixtures and comparison are test_null_gpu's: chromosomes of 3,000 / 5 / 1,200 SNPs, R = 37, seed 5, EVERY
record of every task compared, integer fields and validity exact, T within golden_util.close with that file's
1e-2 floor.  m in {1, 2, 63, 64, 65, 129, 700} x b in {2, 7, 63, 64, 65, 700}: lane and row boundaries (a row
is 64 draws), rounds of 128 blocks that end inside the kept rows (b = 2: every 4 rows) and after them (b = 7:
row 14 = draw 896 > 700, so one round), the cut last block, b > m, b = m, 700 draws = 11 rows past the 8 kept
in registers, and pool 2's 1,200 SNPs so that most 700-blocks wrap.  Pool 1 (5 SNPs) takes the real modulo:
every block longer than 5 goes round the pool; pool -1 crosses chromosome ends."""
import csv
import ctypes as C
import os

import numpy as np
import pytest

import golden_util as gu
import null_util as U
import test_null_gpu as G
from oracle import sfs_oracle as O
from sfs2d import _lib as L
from sfs2d import null as N

pytestmark = pytest.mark.gpu

R, SEED, W, VT = G.R, G.SEED, G.W, G.VT
BLOCKS = [2, 7, 63, 64, 65, 700]
_TWIN = {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SFS2D_GW", "SFS2D_FUSED", "SFS2D_FST_SCAN", "SFS2D_SEG", "SFS2D_TILE"):
        monkeypatch.delenv(k, raising=False)


def _twin(n1p, n2p, block, fold=True, vt=None, start=None, end=None, bg=None, pools=(0, 2)):
    """The expected records of G._tasks(pools) at block length ``block`` (computed once per configuration).
    bg: None = each pool's own chromosome; "int" / "norm" = chromosome 0's background."""
    key = (n1p, n2p, block, fold, vt, start, end, bg, pools)
    if key not in _TWIN:
        p = G._genome(n1p, n2p)
        cfg = O.Cfg(n1p, n2p, vt, fold, start, end)
        bgs = O.chrom_backgrounds(p, cfg)
        if bg == "norm":
            one = tuple(O.normalize(np.asarray(x).ravel()).reshape(np.asarray(x).shape) for x in bgs[0])
        elif bg == "int":
            one = bgs[0]
        bg_of = (lambda c: bgs[c]) if bg is None else (lambda c: one)
        recs = U.oracle_records(*N.resample(p, G._tasks(pools), R, SEED, block=block), cfg, bg_of)
        _TWIN[key] = (recs, None if bg is None else one)
    return _TWIN[key]


def _block_records(p, cfg, tasks, block, bg=None, kernel=None, seed=SEED, reps=R):
    eng = G._engine()
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
            pl.null_run(tasks, reps, seed, block=block)
            return pl.null_read()
        finally:
            pl.close()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------- record parity

@pytest.mark.parametrize("block", BLOCKS)
def test_record_parity_matrix(monkeypatch, block):
    """Every m x this block length, pools 0 and 2, (18, 14), fused, folded."""
    monkeypatch.setenv("SFS2D_FUSED", "1")
    want, _ = _twin(18, 14, block)
    got = _block_records(G._genome(18, 14), G._cfg(18, 14, bg_mode=L.BG_PER_CHROM), G._tasks((0, 2)), block, kernel="k_scan_w")
    assert G._check(got, want) > len(want)


@pytest.mark.parametrize("size,flavour,fold", [((18, 14), "sliced", True), ((18, 14), "fused", False), ((3, 2), "fused", True),
                                               ((100, 75), "gw", True), ((100, 75), "g", True)])
def test_record_parity_grids(monkeypatch, size, flavour, fold):
    """One block length (65: a row spans two blocks) on every way a plan leaves its tables, not folded, the
    smallest grid, and the large grid's kernels."""
    env, kernel = G.FLAVOURS[flavour]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n1p, n2p = size
    pools = (2,) if size == (100, 75) else (0, 2)   # (the oracle takes 25 ms per record of a 101 x 76 grid)
    want, _ = _twin(n1p, n2p, 65, fold, pools=pools)
    got = _block_records(G._genome(n1p, n2p), G._cfg(n1p, n2p, fold=fold, bg_mode=L.BG_PER_CHROM), G._tasks(pools), 65,
                         kernel=kernel)
    assert G._check(got, want) > len(want)


def test_record_parity_variant_type():
    """A drawn SNP that the variant_type filter excludes stays out of the spectra, counts toward m and its
    block, and not toward snp_count."""
    p = G._genome(18, 14)
    want, _ = _twin(18, 14, 65, vt=VT)
    got = _block_records(p, G._cfg(18, 14, bg_mode=L.BG_PER_CHROM, ann_want=p.ann_names.index(VT)), G._tasks((0, 2)), 65)
    G._check(got, want)
    big = got[got["end"] == 700]
    assert np.all(big["snp_count"] < 700) and np.all(big["snp_count"] > 100) and np.all(big["n2_all"] <= big["snp_count"])


def test_record_parity_position_filter():
    p = G._genome(18, 14)
    start, end = int(p.pos[700]), int(p.pos[2300])
    want, _ = _twin(18, 14, 65, start=start, end=end)
    got = _block_records(p, G._cfg(18, 14, bg_mode=L.BG_PER_CHROM, start_position=start, end_position=end), G._tasks((0, 2)), 65)
    G._check(got, want)
    big = got[got["end"] == 700]
    assert np.all(big["snp_count"] == 700) and np.all(big["n2_all"] < 700)


def test_record_parity_sliding_plan():
    want, _ = _twin(18, 14, 65)
    got = _block_records(G._genome(18, 14), G._cfg(18, 14, bg_mode=L.BG_PER_CHROM, step=W // 4, fst=True), G._tasks((0, 2)), 65)
    G._check(got, want)


@pytest.mark.parametrize("block", [7, 700])
@pytest.mark.parametrize("kind", ["int", "norm"])
def test_record_parity_supplied_background(kind, block):
    """One supplied table for every pool, the 5-SNP pool 1 (blocks of 7 and 700 go round it once and 140 times)
    and pool -1: one circle over all 4,205 SNPs, whose blocks cross chromosome ends."""
    p = G._genome(18, 14)
    want, bg = _twin(18, 14, block, bg=kind, pools=(1, -1))
    cfg = G._cfg(18, 14, bg_mode=L.BG_SUPPLIED) if kind == "int" else G._cfg(18, 14, bg_mode=L.BG_SUPPLIED,
                                                                             window_mode=L.WINDOW_SNPS, window=50)
    got = _block_records(p, cfg, G._tasks((1, -1)), block, bg=bg)
    G._check(got, want)
    assert np.all(got["chrom"][: len(G.MS) * R] == 1) and np.all(got["chrom"][len(G.MS) * R:] == 0xFFFFFFFF)
    if block == 700:   # the twin's pool -1 windows do cross chromosome ends (3,000 | 5 | 1,200 SNPs)
        d = N.draw_indices(SEED, -1, 0, p.n, 700, R, block=700)
        assert np.any((d.min(axis=1) < 3000) & (d.max(axis=1) >= 3005)) and np.any(d[:, -1] < d[:, 0])


def test_record_parity_wide_bins():
    """m = 65,536 takes 32-bit 2D bins; 16 blocks of 4,096 over pool 2's 1,200 SNPs: each goes round it."""
    p = G._genome(3, 2)
    cfg = O.Cfg(3, 2)
    bgs = O.chrom_backgrounds(p, cfg)
    want = U.oracle_records(*N.resample(p, [(2, 65536)], 2, SEED, block=4096), cfg, lambda c: bgs[c])
    got = _block_records(p, G._cfg(3, 2, bg_mode=L.BG_PER_CHROM), [(2, 65536)], 4096, reps=2)
    G._check(got, want, wide=True)


# ------------------------------------------------------------------------------------------- block 1, independence

def _run_blocks(eng, pl, tasks, reps, seed, block, out=None):
    """sfs2d_plan_null_run_blocks itself (Plan.null_run sends block 1 to sfs2d_plan_null_run)."""
    tk = np.ascontiguousarray(np.asarray(tasks, np.int64).reshape(-1, 2))
    npar = L.NullParams(seed=seed, replicates=reps)
    rc = eng.lib.sfs2d_plan_null_run_blocks(pl.h, C.byref(npar), block, L.ptr(tk), len(tk), out)
    if rc == 0:
        pl._null_call_n, pl._null_parts, pl._null_dev = len(tk) * reps, [], False
    return rc


def test_block_one_is_k_null_byte_for_byte():
    p = G._genome(18, 14)
    tasks = G._tasks((0, 2))
    eng = G._engine()
    dev = eng.upload(p)
    try:
        pl = eng.plan(dev, G._cfg(18, 14, bg_mode=L.BG_PER_CHROM))
        try:
            pl.run()
            pl.check()
            pl.null_run(tasks, R, SEED)
            a = pl.null_read()
            assert _run_blocks(eng, pl, tasks, R, SEED, 1) == 0
            b = pl.null_read()
            pl.null_run(tasks, R, SEED, block=1)
            c = pl.null_read()
            pl.null_run(tasks, R, SEED, block=2)
            d = pl.null_read()
        finally:
            pl.close()
    finally:
        dev.close()
    assert len(a) == len(tasks) * R and a.tobytes() == b.tobytes() == c.tobytes()
    assert d.tobytes() != a.tobytes() and np.array_equal(d["end"], a["end"])


def test_records_depend_on_the_task_alone(monkeypatch):
    import torch
    p = G._genome(18, 14)
    tasks = G._tasks((0, 2))
    B = 65
    eng = G._engine()
    dev = eng.upload(p)
    try:
        pl = eng.plan(dev, G._cfg(18, 14, bg_mode=L.BG_PER_CHROM))
        try:
            pl.run()
            pl.check()
            pl.null_run(tasks, R, SEED, block=B)
            a = pl.null_read()
            pl.null_run(tasks[::-1], R, SEED, block=B)
            b = pl.null_read()
            pl.null_run(tasks[:5], R, SEED, block=B)
            c1 = pl.null_read()
            pl.null_run(tasks[5:], R, SEED, block=B)
            c2 = pl.null_read()
            pl.null_run(tasks, 5, SEED, block=B)     # fewer replicates: the same first five
            e = pl.null_read()
            pl.null_run(tasks, R, SEED, block=700)   # for m <= 65 any block >= m is the same single run
            h = pl.null_read()
            monkeypatch.setattr(N, "MAX_CALL_RECORDS", 3 * R)
            pl.null_run(tasks, R, SEED, block=B)
            f = pl.null_read()
            buf = torch.zeros(len(tasks) * R * 64, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            pl.null_run(tasks, R, SEED, out_dev_ptr=buf.data_ptr(), block=B)
            pl.check()
            g = buf.cpu().numpy().view(L.WINDOW_DTYPE)
        finally:
            pl.close()
    finally:
        dev.close()
    by_task = lambda x: x.reshape(-1, R)
    assert by_task(a).tobytes() == by_task(b)[::-1].tobytes()
    assert a.tobytes() == np.concatenate([c1, c2]).tobytes()
    assert e.tobytes() == by_task(a)[:, :5].tobytes()
    assert f.tobytes() == a.tobytes() and g.tobytes() == a.tobytes()
    small = np.array([m for _, m in tasks]) <= 65
    assert by_task(a)[small].tobytes() == by_task(h)[small].tobytes()
    assert by_task(a)[~small].tobytes() != by_task(h)[~small].tobytes()


# ------------------------------------------------------------------------------------------- plan untouched

@pytest.mark.parametrize("flavour", ["sliced", "fused", "gw", "supplied"])
def test_block_null_run_leaves_the_plan_as_it_found_it(monkeypatch, flavour):
    size = (100, 75) if flavour == "gw" else (18, 14)
    if flavour in G.FLAVOURS:
        for k, v in G.FLAVOURS[flavour][0].items():
            monkeypatch.setenv(k, v)
    p = G._genome(*size)
    eng = G._engine()
    dev = eng.upload(p)
    try:
        pl = eng.plan(dev, G._cfg(*size, bg_mode=L.BG_SUPPLIED if flavour == "supplied" else L.BG_PER_CHROM, fst=True))
        try:
            if flavour == "supplied":
                pl.set_background(*O.chrom_backgrounds(p, O.Cfg(*size))[0])
            pl.run()
            pl.check()
            recs, fst = pl.read(), pl.read_fst()
            assert len(recs) > 10 and np.isfinite(fst).any()
            pool = 1 if flavour == "supplied" else 2
            pl.null_run([(pool, 64), (0, 700)], 9, SEED, block=7)
            first = pl.null_read()
            for _ in range(2):
                pl.run()
                pl.check()
                assert pl.read().tobytes() == recs.tobytes() and pl.read_fst().tobytes() == fst.tobytes()
            pl.null_run([(pool, 64), (0, 700)], 9, SEED, block=7)
            assert pl.null_read().tobytes() == first.tobytes()
        finally:
            pl.close()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------- refusals

def test_refusals():
    from sfs2d.synth import synth_genome
    p = synth_genome(3, [400, 0, 300], 18, 14, seed=3)               # chromosome 1 is empty
    eng = G._engine()
    dev = eng.upload(p)

    def refused(pl, tasks, block, reps=3):
        with pytest.raises(L.Sfs2dError) as ei:
            pl.null_run(tasks, reps, SEED, block=block)
        assert ei.value.code == L.E_ARG and len(str(ei.value)) > len("sfs2d error -1: ")
        return str(ei.value)
    try:
        pl = eng.plan(dev, G._cfg(18, 14, bg_mode=L.BG_PER_CHROM))
        try:
            att = pl.attach(G._cfg(18, 14, bg_mode=L.BG_PER_CHROM, window=2 * W))
            assert "run" in refused(pl, [(0, 5)], 4)                 # sfs2d_plan_null_run's refusals hold
            pl.run()
            pl.check()
            for bad in (0, -1, 1 << 32):
                assert "block" in refused(pl, [(0, 5)], bad)
            assert "-1" in refused(pl, [(-1, 5)], 4)
            assert "empty" in refused(pl, [(1, 5)], 4)
            assert "m must" in refused(pl, [(0, 0)], 4)
            assert "replicates" in refused(pl, [(0, 5)], 4, reps=0)
            assert "attached" in refused(att, [(0, 5)], 4)
            pl.null_run([(0, 5), (2, 6)], 3, SEED, block=(1 << 32) - 1)   # the longest block
            assert len(pl.null_read()) == 6
        finally:
            pl.close()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------- end to end

def _expected_p(p, cfg, windows_by_label, rows_by_size, reps, seed, block):
    """null.pvalues over oracle twins, as test_null_gpu._expected_p, the null drawn in blocks."""
    bgs = O.chrom_backgrounds(p, cfg)
    bg_of = lambda c: bgs[c]
    wins = [w for key in rows_by_size for lb, w in windows_by_label[key].items() if lb in rows_by_size[key]]
    obs = U.oracle_records(p, wins, cfg, bg_of, wid_of=lambda w: 0)
    cls = N.size_classes(obs["end"])
    tasks = sorted(set(zip(obs["chrom"].tolist(), cls.tolist())))
    null = U.oracle_records(*N.resample(p, tasks, reps, seed, block=block), cfg, bg_of)
    pv = N.pvalues(obs, null, cls)
    out, k = {}, 0
    for key in rows_by_size:
        for lb in windows_by_label[key]:
            if lb in rows_by_size[key]:
                out[(key, lb)] = {name: (None if np.isnan(pv[name][k]) else float(pv[name][k])) for name in N.P_KEYS}
                k += 1
    assert k == len(obs)
    return out, len(tasks)


def test_scan_pvalues_blocks_end_to_end():
    import twoDSFS_class as T
    from sfs2d.synth import synth_genome
    p = synth_genome(2, [2500, 1500], 18, 14, seed=21)
    cfg = O.Cfg(18, 14)
    names = p.chrom_names
    obj = T.LikelihoodInference_jointSFS(None, None, pop1=p.pop1, pop2=p.pop2, pop1_size=18, pop2_size=14)
    reps, seed = 29, 3
    plain = obj.multi_scan(p, (8000,), (40,))
    labels = {8000: {f"{names[c]} {s}-{s + 7999}": (c, b, e) for c, s, b, e in O.bp_windows(p, 8000)},
              "40snps": {f"{names[c]} {s}-{ep}": (c, b, e) for c, s, ep, b, e in O.snp_windows(p, 40)[0]}}
    seen = {}
    for block, length in ((10, 10), ("window", (1 << 32) - 1), (None, 1)):
        got = obj.scan_pvalues(p, window_sizes=(8000,), snp_window_sizes=(40,), replicates=reps, seed=seed, block=block)
        assert list(got) == list(plain) == [8000, "40snps"]
        want, ntasks = _expected_p(p, cfg, labels, got, reps, seed, length)
        assert ntasks > 5
        for key in got:
            assert G._strip(got[key]) == plain[key] and len(got[key]) > 20
            for lb, row in got[key].items():
                assert {k: row[k] for k in N.P_KEYS} == want[(key, lb)], (block, key, lb)
        seen[block] = [row["p_T2D"] for rows in got.values() for row in rows.values()]
    assert seen[10] != seen[None] and seen["window"] != seen[None] and seen["window"] != seen[10]
    with pytest.raises(ValueError, match="block"):
        obj.scan_pvalues(p, window_sizes=(8000,), block="chromosome")
    with pytest.raises(ValueError, match="block"):
        obj.scan_pvalues(p, window_sizes=(8000,), block=0)


def test_cli_null_block(tmp_path):
    """--null-block 10 writes the p_* columns of scan_pvalues(block=10); without it every file is what the
    drivers write today (no option: multi_scan; --null-replicates alone: scan_pvalues' single-SNP null)."""
    import twoDSFS_class as T
    from sfs2d import cli
    from sfs2d.vcf import read_vcf
    vcf, pm = os.path.join(gu.GOLD, "vcf_test.vcf.gz"), os.path.join(gu.GOLD, "popmap_3pop.txt")
    base = [vcf, pm, "--pop1", "uv", "--pop2", "bv", "--pop1-size", "11", "--pop2-size", "11", "--fst",
            "--window", "500000", "--snp-window", "100"]
    nul = ["--null-replicates", "49", "--null-seed", "4"]
    plain = cli.main(base + ["--out-prefix", str(tmp_path / "plain")])
    single = cli.main(base + nul + ["--out-prefix", str(tmp_path / "single")])
    blocks = cli.main(base + nul + ["--null-block", "10", "--out-prefix", str(tmp_path / "blocks")])
    window = cli.main(base + nul + ["--null-block", "window", "--out-prefix", str(tmp_path / "window")])
    assert [os.path.basename(o) for o in blocks] == ["blocks_500kb.csv", "blocks_100snps.csv"]
    p = read_vcf(vcf, pm).to_packed("uv", "bv")
    obj = T.LikelihoodInference_jointSFS(vcf, pm, pop1_size=11, pop2_size=11)
    keys = (500000, "100snps")
    fst100 = obj.window_fst(p, snp_window_size=100)

    def reference(res, key, null):
        ref = str(tmp_path / "ref.csv")
        cli.write_csv(ref, res[key], {}, res["fst"][key] if key != "100snps" else fst100, None, null)
        return open(ref, "rb").read()
    res = obj.multi_scan(p, [500000], [100], fst=True)
    for path, key in zip(plain, keys):
        assert open(path, "rb").read() == reference(res, key, False)
    for paths, block in ((single, None), (blocks, 10), (window, "window")):
        kw = {} if block is None else {"block": block}
        res = obj.scan_pvalues(p, [500000], [100], fst=True, replicates=49, seed=4, **kw)
        for path, key in zip(paths, keys):
            assert open(path, "rb").read() == reference(res, key, True), (block, key)
    differ = 0
    for a, b in zip(single, blocks):
        with open(a, newline="") as fa, open(b, newline="") as fb:
            ra, rb = list(csv.DictReader(fa)), list(csv.DictReader(fb))
        assert list(rb[0]) == T.col_names + ["FST"] + cli.P_COLS and len(ra) == len(rb) > 0
        for x, y in zip(ra, rb):
            assert {k: v for k, v in x.items() if k not in cli.P_COLS} == {k: v for k, v in y.items() if k not in cli.P_COLS}
            assert (y["p_T2D"] == "") == (y["T2D"] == "")
            differ += x["p_T2D"] != y["p_T2D"]
    assert differ > 0
