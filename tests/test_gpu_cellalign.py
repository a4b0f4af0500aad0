"""svg_cell_align_batch (the vote, then cellCounts_select_and_write_alignments up to the writer,
cell-counts.c:2648-2719, on the GPU) through VoteIndex.cell_align: byte-equal to the reference's
own answers (tests/golden/cellalign/cellalign.npz) on every case, and to the plain-C model
(tests/native/cellalign_model.c, itself pinned to the reference by tests/test_cellalign_golden.py)
on 20k simulated reads with and without exons; the same answers however the batch is cut; the
refusals of the entry point."""
import numpy as np
import pytest

from tests.cellalign_common import CASES, case_params, golden_case, host_index, make_exons, model_align, raw
from tests.common import ensure_built

ensure_built()
pytestmark = pytest.mark.gpu

CHUNK = 1 << 17   # reads per chunk of the host entry (svg_cell_align.hip, CH)
IDS = ["%s-n%d-%s" % c for c in CASES]


@pytest.fixture(scope="module")
def open_index(index_cache):
    import subread_amd as sa
    held = {}

    def get(key):
        if key not in held:
            held[key] = sa.VoteIndex(index_cache.get(key), device=0)
        return held[key]

    yield get
    for ix in held.values():
        ix.close()


def same(got, want):
    return (len(got[0]) == len(want[0]) and len(got[1]) == len(want[1]) and (raw(got[0]) == raw(want[0])).all()
            and (raw(got[1]) == raw(want[1])).all())


@pytest.mark.parametrize("key,total,which", CASES, ids=IDS)
def test_gpu_cell_align_matches_reference(key, total, which, open_index):
    pk, ea, eb, heads, alns = golden_case(key, total, which)
    ix = open_index(key)
    ix.set_cell_exons(ea, eb)
    try:
        got = ix.cell_align(pk, **case_params(total, which))
    finally:
        ix.set_cell_exons([], [])
    assert (raw(got[0]) == raw(heads)).all()
    assert len(got[1]) == len(alns) and (raw(got[1]) == raw(alns)).all()


@pytest.fixture(scope="module")
def sim_reads(index_cache):
    """20k simulated 100-base reads of synth4242 (1% substitutions, some indels, some N), packed"""
    import subread_amd as sa
    from subread_amd.sim import Genome, simulate_reads
    g = Genome.read_fasta(index_cache.genome_fasta("synth4242"))
    rb = simulate_reads(g, 20000, 100, seed=2648, indel=0.05, nrate=0.002, threads=8)
    return rb, sa.pack_reads(rb), len(g.flat)


def exon_list(glen, seed):
    return make_exons(glen, np.random.default_rng(seed))


@pytest.fixture(scope="module")
def model_answers(sim_reads, index_cache):
    out, hosts = {}, {}

    def get(key, exon_seed=None):
        if (key, exon_seed) not in out:
            if key not in hosts:
                hosts[key] = host_index(index_cache.get(key))
            ex = exon_list(sim_reads[2], exon_seed) if exon_seed is not None else None
            out[key, exon_seed] = model_align(hosts[key], sim_reads[0], ex)
        return out[key, exon_seed]

    return get


@pytest.mark.parametrize("key", ["synth4242_full", "synth4242_gapped"])
def test_gpu_cell_align_matches_model_at_volume(key, open_index, sim_reads, model_answers):
    """without exons, with a list, and with a different list: each the model's answers"""
    ix = open_index(key)
    want = model_answers(key)
    assert same(ix.cell_align(sim_reads[1]), want)
    assert (want[0]["n_records"] > 0).mean() > (0.5 if "full" in key else 0.2)
    try:
        seen = []
        for seed in (11, 12):
            ix.set_cell_exons(*exon_list(sim_reads[2], seed))
            w = model_answers(key, seed)
            assert same(ix.cell_align(sim_reads[1]), w)
            seen.append(w[1]["score"])
        assert len(seen[0]) != len(seen[1]) or (seen[0] != seen[1]).any()   # the second list changed the answers
        assert (seen[0] >= 10 ** 12).any() and (seen[0] < 10 ** 12).any()
    finally:
        ix.set_cell_exons([], [])
    assert same(ix.cell_align(sim_reads[1]), want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_gpu_cell_align_batch_split_invariance(n, open_index, sim_reads, model_answers):
    """the first n reads alone, back to back and strided, give the first n reads' answers"""
    import subread_amd as sa
    want = model_answers("synth4242_full")
    k = int(want[0]["n_records"][:n].sum())
    wh = want[0][:n].copy()
    wa = want[1][:k]
    ix = open_index("synth4242_full")
    sub = sim_reads[0].slice(0, n)
    assert same(ix.cell_align(sa.pack_reads(sub)), (wh, wa))
    assert same(ix.cell_align(sa.pack_reads(sub, stride=112)), (wh, wa))


def test_gpu_cell_align_one_past_the_chunk(open_index, sim_reads, model_answers):
    """CHUNK + 1 reads, the 20k simulated reads over and over: the second round of the host entry's
    chunk loop is one read (its read offset, the record base of the scan and the compaction, the
    growth of the result arrays).  Every read's head and records are those of its source read."""
    import subread_amd as sa
    from subread_amd.abi import ReadBatch
    want = model_answers("synth4242_full")
    rb = sim_reads[0]
    n = CHUNK + 1
    idx = np.arange(n) % len(rb)
    big = ReadBatch(np.ascontiguousarray(rb.seq[:100 * len(rb)].reshape(len(rb), 100)[idx]).reshape(-1),
                    np.arange(n, dtype=np.uint64) * 100, np.full(n, 100, np.uint16))
    assert (rb.lens == 100).all() and (rb.offsets == np.arange(len(rb), dtype=np.uint64) * 100).all()
    heads, alns = open_index("synth4242_full").cell_align(sa.pack_reads(big, threads=16))
    wh = want[0][idx]
    assert len(heads) == n and (heads["n_records"] == wh["n_records"]).all()
    assert (heads["multi_alignment_no"] == wh["multi_alignment_no"]).all()
    has = heads["n_records"] > 0
    assert has[CHUNK - 1] or has[CHUNK] or has[:CHUNK].any()
    assert (heads["first_record"][has] == (np.cumsum(heads["n_records"]) - heads["n_records"])[has]).all()
    assert not heads["first_record"][~has].any()
    src = want[0]["first_record"][idx][has]            # (one record per mapped read at the defaults)
    assert (heads["n_records"] <= 1).all() and len(alns) == len(src) and (raw(alns) == raw(want[1][src])).all()


def test_gpu_cell_align_empty_and_short(open_index):
    import subread_amd as sa
    from subread_amd.abi import ReadBatch
    ix = open_index("synth4242_full")
    h, a = ix.cell_align(sa.pack_reads(ReadBatch.from_list([])))
    assert len(h) == 0 and len(a) == 0
    pk = golden_case(*CASES[6])[0]
    whole = ix.cell_align(pk)
    short = pk.lens < 16
    assert short.any() and not raw(whole[0][short]).any()


def test_gpu_cell_align_refusals(open_index, index_cache):
    import subread_amd as sa
    ix = open_index("synth4242_full")
    pk = golden_case(*CASES[6])[0]
    for bad in (dict(total_subreads=6), dict(total_subreads=21), dict(max_indel_length=4), dict(min_votes_per_mapped_read=0),
                dict(min_votes_per_mapped_read=65), dict(max_differential_from_top_vote_number=0),
                dict(max_differential_from_top_vote_number=31), dict(max_mismatching_bases_in_reads=-1),
                dict(max_mismatching_bases_in_reads=101), dict(min_mapped_length_for_mapped_read=-2),
                dict(min_mapped_length_for_mapped_read=161), dict(max_reported_alignments_per_read=0),
                dict(max_reported_alignments_per_read=31)):
        with pytest.raises(sa.SvgError, match="SVG_E_ARG"):
            ix.cell_align(pk, **bad)
    with pytest.raises(sa.SvgError, match="SVG_E_ARG"):
        ix.set_cell_exons([10], [5])
    multi = sa.VoteIndex(index_cache.get("synth4242_fullM1"), device=0)
    try:
        assert multi.n_blocks > 1
        with pytest.raises(sa.SvgError, match="SVG_E_UNSUPPORTED"):
            multi.cell_align(pk)
        with pytest.raises(sa.SvgError, match="SVG_E_UNSUPPORTED"):
            multi.set_cell_exons([100], [200])
    finally:
        multi.close()
