"""svg_cell_vote_batch (cellCounts' voting step on the GPU, cell-counts.c:3051-3131 and
:2786-2881) through VoteIndex.cell_vote: byte-equal to the reference's own tables
(tests/golden/cellvote/cellvote.npz) on full and gapped indexes with 7, 10 and 20 subreads, and to
the plain-C model (tests/native/cellvote_model.c, itself pinned to the reference by
tests/test_cellvote_golden.py) on 20k simulated reads and on batches of more than one and more than two chunks of the host
entry; the same answers however the batch is cut;
the refusals of the entry point."""
import numpy as np
import pytest

from tests.cellvote_common import CASES, golden_case, model_vote, model_vote_sliced, raw, unpack_ascii
from tests.common import ensure_built

ensure_built()
pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("key,total", CASES)
def test_gpu_cell_vote_matches_reference(key, total, open_index):
    pk, heads, slots, _ = golden_case(key, total)
    got = open_index(key).cell_vote(pk, total_subreads=total)
    assert (raw(got[0]) == raw(heads)).all()
    assert len(got[1]) == len(slots) and (raw(got[1]) == raw(slots)).all()


@pytest.fixture(scope="module")
def sim_reads(index_cache):
    """20k simulated 100-base reads of synth4242 (1% substitutions, some indels, some N), packed"""
    import subread_amd as sa
    from subread_amd.sim import Genome, simulate_reads
    g = Genome.read_fasta(index_cache.genome_fasta("synth4242"))
    rb = simulate_reads(g, 20000, 100, seed=3051, indel=0.05, nrate=0.002, threads=8)
    return rb, sa.pack_reads(rb)


@pytest.fixture(scope="module")
def model_answers(sim_reads, open_index):
    out = {}

    def get(key):
        if key not in out:
            out[key] = model_vote(open_index(key).export(), sim_reads[0], 10)
        return out[key]

    return get


@pytest.mark.parametrize("key", ["synth4242_full", "synth4242_gapped"])
def test_gpu_cell_vote_matches_model_at_volume(key, open_index, sim_reads, model_answers):
    want = model_answers(key)
    got = open_index(key).cell_vote(sim_reads[1])
    assert same(got, want)
    assert (want[0]["max_vote"] >= 2).mean() > 0.5   # most reads find their place


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_gpu_cell_vote_batch_split_invariance(n, open_index, sim_reads, model_answers):
    """the first n reads alone, as strided and as back-to-back packed reads, give the first n
    reads' tables of the whole batch"""
    import subread_amd as sa
    heads, slots = model_answers("synth4242_full")
    k = int(heads["n_slots"][:n].sum())
    want = (heads[:n], slots[:k])
    ix = open_index("synth4242_full")
    part = sim_reads[0].slice(0, n)
    assert same(ix.cell_vote(sa.pack_reads(part)), want)
    assert same(ix.cell_vote(sa.pack_reads(part, stride=112)), want)


CHUNK = 1 << 17   # reads per chunk of svg_cell_vote_batch's host entry (svg_cell.hip)


@pytest.fixture(scope="module")
def chunk_reads(index_cache, open_index):
    """2 * CHUNK + 1 simulated 100-base reads (substitutions, indels, N bases) and the model's
    tables for them, first_slot counted across the whole batch"""
    from subread_amd.sim import Genome, simulate_reads
    g = Genome.read_fasta(index_cache.genome_fasta("synth4242"))
    rb = simulate_reads(g, 2 * CHUNK + 1, 100, seed=131073, indel=0.05, nrate=0.002, threads=16)
    return rb, model_vote_sliced(open_index("synth4242_full").export(), rb, 10)


@pytest.mark.parametrize("stride", [None, 112])
@pytest.mark.parametrize("n", [CHUNK + 1, 2 * CHUNK + 1])
def test_gpu_cell_vote_across_chunks(n, stride, open_index, chunk_reads):
    """batches that take the host entry's chunk loop past its first round (one read into the
    second chunk; two full chunks and one read), back to back and strided: the later chunks' read
    offsets, the slot base of the scan and the compaction, the growth of the result arrays"""
    import subread_amd as sa
    rb, (heads, slots) = chunk_reads
    k = int(heads["n_slots"][:n].sum())
    got = open_index("synth4242_full").cell_vote(sa.pack_reads(rb.slice(0, n), stride=stride, threads=16))
    assert same(got, (heads[:n], slots[:k]))
    assert int(got[0]["first_slot"][n - 1]) == k - int(heads["n_slots"][n - 1]) > 0


def test_gpu_cell_vote_empty_batch(open_index):
    import subread_amd as sa
    from subread_amd.abi import ReadBatch
    heads, slots = open_index("synth4242_full").cell_vote(sa.pack_reads(ReadBatch.from_list([])))
    assert len(heads) == 0 and len(slots) == 0


def test_gpu_cell_vote_refusals(open_index, index_cache):
    import subread_amd as sa
    from subread_amd.abi import ReadBatch
    ix = open_index("synth4242_full")
    ok = sa.pack_reads(ReadBatch.from_list([b"ACGT" * 40]))
    assert len(ix.cell_vote(ok)[0]) == 1
    with pytest.raises(sa.SvgError, match="SVG_E_ARG"):
        ix.cell_vote(sa.pack_reads(ReadBatch.from_list([b"ACGT" * 40, b"ACGT" * 40 + b"A"])))
    for t in (6, 21):
        with pytest.raises(sa.SvgError, match="SVG_E_ARG"):
            ix.cell_vote(ok, total_subreads=t)
    with pytest.raises(sa.SvgError, match="SVG_E_ARG"):
        ix.cell_vote(ok, max_indel_length=6)
    multi = sa.VoteIndex(index_cache.get("synth4242_fullM1"), device=0)
    try:
        assert multi.n_blocks > 1
        with pytest.raises(sa.SvgError, match="SVG_E_UNSUPPORTED"):
            multi.cell_vote(ok)
    finally:
        multi.close()
