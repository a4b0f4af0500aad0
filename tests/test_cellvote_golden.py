"""CPU: the cellCounts voting fixtures (tests/golden/cellvote/cellvote.npz, written by the
reference's own prefill_votes and cellCounts_process_copy_ptrs_to_votes, see
make_cellvote_golden.py) reach the edges of the tally, and the plain-C model
(tests/native/cellvote_model.c) reproduces every byte of them."""
import numpy as np
import pytest

from tests.cellvote_common import (CASES, edge_counts, golden_case, host_index, index_runs, long_run_bar, model_vote,
                                   raw, unpack_ascii)
from tests.common import ensure_built

ensure_built()


EDGES = ("row_full", "both_masks", "toli6", "neighbour_row", "long_run")


@pytest.mark.parametrize("key,total", CASES)
def test_golden_tables_reach_the_edges(key, total, index_cache):
    """Every case holds at least 20 reads with each of: a row at 3 items; slots of both masks in
    one table; a slot with toli >= 6; a slot voted for through a +-5 neighbour row (a recorded
    distance d with (pos + d) / 5 % 17 other than the slot's row); a hit list longer than 64.

    The last one cannot be had on three of the four indexes: a hit list is an equal-key run of the
    index, and the longest run of chr901_gapped has 60 items, of synth4242_full 63, of
    synth4242_gapped 27 (the builder leaves out 16-mers of 100 copies or more, and a gapped index
    holds every third position).  The test measures the index's longest run itself; where it is at
    most 64 the bar is a hit list of more than half of that longest run instead."""
    pk, heads, slots, max_run = golden_case(key, total)
    assert int(heads["n_slots"].sum()) == len(slots)
    short = pk.lens < 16
    assert (heads["first_slot"] == np.cumsum(heads["n_slots"]) - heads["n_slots"])[~short].all()
    assert short.any() and not raw(heads[short]).any()      # skipped reads: a zero head
    assert (heads["applied_subreads"][~short] >= 1).all() and heads["applied_subreads"].max() <= total
    if total == 20:
        assert heads["applied_subreads"].max() == 20
    assert pk.xmask is not None                              # N bases
    assert {16, 17, 18, 19, 31, 50, 100, 160} <= set(int(x) for x in pk.lens)
    longest = int(index_runs(host_index(index_cache.get(key)))[1].max())
    assert (longest > 64) == (key == "chr901_full")
    assert int(max_run.max()) <= longest
    got = edge_counts(heads, slots, max_run)
    got["long_run"] = int((max_run > long_run_bar(longest)).sum())
    for k in EDGES:
        assert got[k] >= 20, (k, got)


@pytest.mark.parametrize("key,total", CASES)
def test_model_equals_reference(key, total, index_cache):
    pk, heads, slots, _ = golden_case(key, total)
    got = model_vote(host_index(index_cache.get(key)), unpack_ascii(pk), total)
    assert got is not None
    assert (raw(got[0]) == raw(heads)).all()
    assert len(got[1]) == len(slots) and (raw(got[1]) == raw(slots)).all()


def test_model_refusals():
    from subread_amd.abi import ReadBatch
    ix = dict(buckets=1, gap=1, bstart=np.zeros(2, np.uint32), keys=np.zeros(1, np.int16), vals=np.zeros(1, np.uint32))
    ok = ReadBatch.from_list([b"A" * 160])
    assert model_vote(ix, ok, 10) is not None
    assert model_vote(ix, ok, 6) is None and model_vote(ix, ok, 21) is None
    assert model_vote(ix, ok, 10, max_indel_length=4) is None
    assert model_vote(ix, ReadBatch.from_list([b"A" * 161]), 10) is None
