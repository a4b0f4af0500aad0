"""svg_cell_counter_* and svg_cell_count_batch (cellCounts' UMI stage on the GPU) through
VoteIndex.cell_counter: equal to the reference's own answers on every fixture case
(tests/golden/cellumi/cellumi.npz) and to the plain-C model (tests/native/cellumi_model.c, pinned to
the reference on the CPU by tests/test_cellumi_golden.py) at volume; finish twice and add after
finish; count_batch against cell_assign + the model on the cellassign fixture's reads; the same
table however the batch is cut; the refusals."""
import numpy as np
import pytest

import subread_amd as sa
from subread_amd.abi import CELL_FEATURE_DTYPE, ReadBatch
from tests.cellassign_common import fixture_allow, fixture_case as assign_case, make_features, make_whitelist, pack_barcodes, raw
from tests.cellumi_common import FIXTURE_CASES, LETTERS, fixture_case, model_run, same_result
from tests.common import ensure_built
from tests.test_cellumi_golden import mask_unknown

ensure_built()
pytestmark = pytest.mark.gpu

KEY = "synth4242_full"


@pytest.fixture(scope="module")
def ix(index_cache):
    x = sa.VoteIndex(index_cache.get(KEY), device=0)
    yield x
    x.close()


@pytest.mark.parametrize("L", [c[0] for c in FIXTURE_CASES])
def test_gpu_add_finish_equals_the_reference(L, ix):
    """entries and counts, every byte; then finish again, and more observations after a finish"""
    obs, want, known = fixture_case(L)
    c = ix.cell_counter(L, 2)
    try:
        n = len(obs[0])
        cut = n // 3
        c.add(*(a[:cut] for a in obs))
        part = c.finish(want_entries=True)
        same_result(part, model_run(*(a[:cut] for a in obs), L))
        c.add(*(a[cut:] for a in obs))
        got = c.finish(want_entries=True)
        same_result(mask_unknown(got, known), want)
        again = c.finish(want_entries=True)
        same_result(again, got)
        assert c.finish()["entries"] is None
        c.reset()
        c.add(*obs)                                  # one add, one finish over everything
        same_result(c.finish(want_entries=True), got)
    finally:
        c.close()


def test_gpu_volume_equals_model(ix):
    """200k observations over two samples, short UMIs of a small alphabet: big sections and merges"""
    rng = np.random.default_rng(4126)
    n, L = 200000, 6
    s, ce, g = rng.integers(0, 3, n), rng.integers(-1, 3, n), rng.integers(0, 5, n) * 400000000
    u = LETTERS[rng.integers(0, 4, (n, L))]
    want = model_run(s, ce, g, u, L)
    e = want["entries"]
    sizes = np.unique(e["sample"].astype(np.int64) << 56 | e["cell"].astype(np.int64) << 32 | e["gene"], return_counts=True)[1]
    assert sizes.max() > 1000 and (e["outcome"] == 1).sum() > 1000      # (the fixture's case L12 holds the section above the LDS list)
    c = ix.cell_counter(L, 2)
    ix.set_timing(True)
    try:
        for k in range(0, n, 70000):
            c.add(s[k:k + 70000], ce[k:k + 70000], g[k:k + 70000], u[k:k + 70000])
        same_result(c.finish(want_entries=True), want)
        t = c.timing()
        assert t["step1_wave"] > 0 and t["sort_rle"] > 0 and t["expand"] == 0
    finally:
        ix.set_timing(False)
        c.close()


def observations_of(heads, hits, genes, bcno, sample_no, umis):
    """one observation per (record, gene of its list) of every read, from cell_assign's arrays"""
    read_of = np.repeat(np.arange(len(heads)), heads["n_records"])
    ok = (hits["contig"] >= 0) & (hits["nhits"] > 0)
    k = hits["nhits"][ok].astype(np.int64)
    rec = np.repeat(np.nonzero(ok)[0], k)
    within = np.arange(len(rec)) - np.repeat(np.cumsum(k) - k, k)
    g = genes[hits["first_gene"][rec].astype(np.int64) + within]
    r = read_of[rec]
    return (np.asarray(sample_no, np.int32)[r], np.asarray(bcno, np.int32)[r], g.astype(np.int64),
            np.asarray(umis, np.uint8).reshape(len(heads), -1)[r])


def pack_umis(umis):
    return sa.pack_reads(ReadBatch.fixed(umis))


@pytest.mark.parametrize("total,which", [(10, "default"), (10, "second")])
def test_gpu_count_batch_on_the_cellassign_fixture(total, which, ix):
    from tests.cellalign_common import case_params
    fc = assign_case(KEY, total, which)
    n, L = len(fc["heads"]), 5
    rng = np.random.default_rng(17 + total)
    umis = LETTERS[np.where(rng.random((n, L)) < 0.02, 4, rng.integers(0, 3, (n, L)))]
    sample_no = rng.integers(0, 3, n).astype(np.int32)
    obs = observations_of(fc["heads"], fc["hits"], fc["genes"], fc["bcno"], sample_no, umis)
    # (the fixture case has 649 reads; the default parameters report one alignment each and forbid two genes)
    assert len(obs[0]) >= 100 and (obs[1] >= 0).sum() >= 50 and (umis == ord("N")).any()
    want = model_run(*obs, L)
    assert len(want["counts"]) >= 20
    p = case_params(total, which)
    ix.set_cell_annotation(fc["features"], allow_multi_overlap=fixture_allow(total, which))
    ix.set_cell_barcodes(fc["whitelist"])
    c, c2, c3 = ix.cell_counter(L, 2), ix.cell_counter(L, 2), ix.cell_counter(L, 2)
    try:
        bpk, upk = pack_barcodes(fc["barcodes"]), pack_umis(umis)
        res = c.count_batch(fc["pk"], bpk, upk, sample_no, want_result=True, **p)
        plain = ix.cell_assign(fc["pk"], bpk, **p)
        assert all(raw(a).tobytes() == raw(b).tobytes() for a, b in zip(res, plain))
        assert c2.count_batch(fc["pk"], bpk, upk, sample_no, **p) is None
        c3.add(*observations_of(*(plain[k] for k in (0, 2, 3, 4)), sample_no, umis))
        for k in (c, c2, c3):
            same_result(k.finish(want_entries=True), want)
        # no barcodes: every observation is dropped for its cell
        c2.reset()
        c2.count_batch(fc["pk"], None, upk, sample_no, **p)
        r = c2.finish()
        assert len(r["counts"]) == 0 and r["dropped_no_cell"] + r["dropped_no_sample"] == len(obs[0])
        # a sample number above n_samples does not fit its field: counted on the device, finish refuses with
        # SVG_E_ARG until reset, whatever else the observation holds (sample 3 without a cell is refused as
        # add refuses it, not dropped), and nothing of it reaches a table
        owner = observations_of(fc["heads"], fc["hits"], fc["genes"], fc["bcno"], np.arange(n), umis)[0]
        over = sample_no.copy()
        over[owner[::7]] = 3
        n_over = int(np.isin(owner, owner[::7]).sum())
        assert n_over >= 10 and (fc["bcno"][owner[::7]] < 0).any() and (fc["bcno"][owner[::7]] >= 0).any()
        for k, bar in ((c2, bpk), (c3, None)):
            k.reset()
            k.count_batch(fc["pk"], bar, upk, over, **p)
            for _ in range(2):
                with pytest.raises(sa.SvgError) as err:
                    k.finish()
                assert err.value.rc == -1 and ("%d observations" % n_over) in str(err.value)
            with pytest.raises(sa.SvgError):
                k.count_batch(fc["pk"], bar, upk, sample_no, **p) or k.finish()     # more observations do not clear it
        with pytest.raises(sa.SvgError) as err:
            c3.add(*(a[owner[::7][:1]] for a in (over, np.full(n, -1), np.zeros(n, np.int64), umis)))   # the same through add
        assert err.value.rc == -1
        c2.reset()
        c2.count_batch(fc["pk"], bpk, upk, sample_no, **p)
        same_result(c2.finish(want_entries=True), want)
    finally:
        ix.set_cell_annotation(np.zeros(0, CELL_FEATURE_DTYPE))
        ix.set_cell_barcodes([])
        for k in (c, c2, c3):
            k.close()


def test_gpu_count_batch_cut_in_two(ix, index_cache):
    """131,073 reads (one more than a chunk) in one call and as two calls: the same table"""
    from subread_amd.sim import Genome, simulate_reads
    n, L = 131073, 12
    g = Genome.read_fasta(index_cache.genome_fasta("synth4242"))
    rb = simulate_reads(g, n, 100, seed=3951, indel=0.02, nrate=0.001, threads=8)
    rng = np.random.default_rng(3951)
    e = ix.export()
    feats = make_features(e["chr_end"][:e["n_chr"]].copy(), int(e["padding"]), rng, per_kb=4.0, genes_per=3)
    wl = make_whitelist(200, 16, rng)
    bc = np.array([np.frombuffer(w, np.uint8) for w in wl])[rng.integers(0, 8, n)]    # few cells: sections large enough for merges
    umis = LETTERS[rng.integers(0, 2, (n, L))]
    sample_no = rng.integers(1, 3, n).astype(np.int32)
    ix.set_cell_annotation(feats, allow_multi_overlap=1)
    ix.set_cell_barcodes(wl)
    a, b = ix.cell_counter(L, 2), ix.cell_counter(L, 2)
    try:
        pk, bpk = sa.pack_reads(rb), pack_umis(bc)
        a.count_batch(pk, bpk, pack_umis(umis), sample_no)
        one = a.finish(want_entries=True)
        heads, _, hits, genes, bcno = ix.cell_assign(pk, bpk)
        same_result(one, model_run(*observations_of(heads, hits, genes, bcno, sample_no, umis), L))
        h = 65536
        for lo, hi in ((0, h), (h, n)):
            b.count_batch(sa.pack_reads(rb.slice(lo, hi)), pack_umis(bc[lo:hi]), pack_umis(umis[lo:hi]), sample_no[lo:hi])
        same_result(b.finish(want_entries=True), one)
        assert len(one["counts"]) >= 1000 and (one["entries"]["outcome"] == 1).sum() >= 100
    finally:
        ix.set_cell_annotation(np.zeros(0, CELL_FEATURE_DTYPE))
        ix.set_cell_barcodes([])
        a.close(), b.close()


def test_gpu_refusals(ix):
    for L, S in ((0, 1), (15, 1), (12, 0), (12, 256)):
        with pytest.raises(sa.SvgError):
            ix.cell_counter(L, S)
    c = ix.cell_counter(4, 2)
    try:
        ok = ([1], [0], [0], [b"ACGT"])
        c.add(*ok)
        for bad in (([3], [0], [0], [b"ACGT"]), ([1], [1 << 24], [0], [b"ACGT"]), ([1], [0], [-1], [b"ACGT"]), ([1], [0], [1 << 31], [b"ACGT"]),
                    ([1], [0], [0], [b"ACGU"]), ([1, 1], [0, 0], [0, 0], [b"AAAA", b"acgt"])):
            with pytest.raises(sa.SvgError):
                c.add(*bad)
        c.add([1, 0, 2], [(1 << 24) - 1, 5, -1], [(1 << 31) - 1, 1, 1], [b"NNNN", b"AAAA", b"CCCC"])
        r = c.finish(want_entries=True)
        assert [tuple(int(v) for v in k) for k in r["counts"]] == [(1, 0, 0, 1), (1, (1 << 24) - 1, (1 << 31) - 1, 1)]   # a refused add appended nothing
        assert r["dropped_no_sample"] == 1 and r["dropped_no_cell"] == 1 and r["entries"]["umi"].tolist() == [b"ACGT", b"NNNN"]
        # the store's growth past the option's bound: SVG_E_NOMEM, and the counter keeps what it had
        sa.lib().svg_set_option(b"cell_count_max_mb", 1)
        n = 70000                                         # 16 bytes each: more than 1 MB
        with pytest.raises(sa.SvgError) as err:
            c.add(np.ones(n), np.zeros(n), np.arange(n), np.tile(np.frombuffer(b"ACGT", np.uint8), (n, 1)))
        assert err.value.rc == -6                       # SVG_E_NOMEM
        sa.lib().svg_set_option(b"cell_count_max_mb", 0)
        assert len(c.finish()["counts"]) == 2
    finally:
        sa.lib().svg_set_option(b"cell_count_max_mb", 0)
        c.close()


def test_gpu_index_close_frees_its_counters(index_cache):
    x = sa.VoteIndex(index_cache.get(KEY), device=0)
    c, d = x.cell_counter(4, 1), x.cell_counter(6, 1)
    c.add([1], [0], [0], [b"ACGT"])
    d.close()
    x.close()
    assert c.c is None and d.c is None
    c.close()
