"""CPU: fragile junction voting of subjunc reads > 160 bp against the REFERENCE's own window tables
(tests/golden/fragile/fragile.npz: every window's finished vote table as core_fragile_junction_voting
hands it to select_best_vote, core-junction.c:5346, its start and length, and the junction it
supported; dumped by oracle/ref_dump_hook.c, SVG_REF_FRAGILE).
  * reach: the reference's own tables show that the fredge read classes (tests/common.py) hit every
    limit of the 30 x 24 table the kernel has code for;
  * the CPU restatement (oracle/svoracle.c svo_fragile_batch) equals the reference window by window;
  * the window layout of every read length 161..1209 equals the reference's two float expressions.
The GPU's comparison with the same dump is tests/test_gpu_fragile.py."""
import numpy as np
import pytest

from tests.common import FREDGE_LENGTHS, ensure_built, fredge_retry_reads
from tests.fragile_common import AMBIGUOUS_CAP, GOLDEN_SETS, PE_LENGTHS, UNKNOWN, assert_equals_reference, fragile_golden

ensure_built()


def _read_of_window(g):
    """the read of every window of g (the dump has one call per long read end, strand by strand:
    calls -> reads through the oracle-independent read order)"""
    ends = 2 if g.reads.r2 is not None else 1
    lens = [g.reads.r1.lens] + ([g.reads.r2.lens] if ends == 2 else [])
    read_of_call = [r for r in range(len(g.reads.r1)) for s in range(2) for e in range(ends) if lens[e][r] > 160]
    return np.array(read_of_call)[g.w["call"]]


def _windows_of_class(g, prefix):
    """indexes of g's windows whose read's class starts with prefix"""
    return np.flatnonzero(np.char.startswith(g.reads.cls[_read_of_window(g)], prefix))


@pytest.fixture(scope="module", params=["fredge_full_se", "fredge_gapped_se"])
def gold(request):
    return fragile_golden(request.param)


def test_golden_note_and_ambiguity_cap():
    for name in GOLDEN_SETS:
        g = fragile_golden(name)
        j = g.w["junction"] == 1
        assert j.sum() > 0
        assert ((g.w["large_side"] == UNKNOWN) & j).sum() <= AMBIGUOUS_CAP * j.sum()
        assert sorted(set(g.w["full_rl"].tolist())) == sorted(FREDGE_LENGTHS if name.endswith("_se") else PE_LENGTHS)
        if g.reads.r2 is not None:
            assert (g.reads.r1.lens != g.reads.r2.lens).all()


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_golden_classes_on_both_strands(name):
    """every class is drawn from both strands (paired: the class's read is r1 of some pairs and r2 of
    others), and the reference reported slots for reads of either strand.  (The dump's
    negative_strand says nothing here: every read is voted on both strands.)  Junctions are another
    matter: in the reference's dump every junction window belongs to a call with negative_strand 0,
    here and in the sj_*_long cases -- core13_test_donor (core-junction.c:5366) accepts none on the
    reversed read -- so only the forward reads of the sj_ classes give any."""
    g = fragile_golden(name)
    for cls in np.unique(g.reads.cls):
        assert set(g.reads.strand[g.reads.cls == cls].tolist()) == {0, 1}, cls
    strand = g.reads.strand[_read_of_window(g)]
    win = np.repeat(np.arange(len(g.w)), g.w["n_used"])
    reported = np.bincount(win[(g.s["votes"] >= g.w["max_vote"][win]) & (g.s["rec"][:, 3] != 0)], minlength=len(g.w)) > 0
    for st in (0, 1):
        assert (reported & (strand == st)).any(), st
        assert (reported & (g.w["negative_strand"] == st)).any(), st
    assert ((g.w["junction"] == 1) & (strand == 0)).any()


def test_reach_full_row_with_drop(gold):
    """a row of 24 on reads whose 16-mers have 25 or more copies: the 25th candidate was dropped"""
    for cls in ("in_t150_25", "in_t150_40", "id_t150_40", "in_edge_first"):
        w = _windows_of_class(gold, cls)
        assert (gold.w["items"][w] == 24).any(), cls


def test_reach_exactly_full_row(gold):
    w = _windows_of_class(gold, "in_t150_24")
    assert (gold.w["items"][w].max(1) == 24).any()
    # (a window that starts late in a unit has one more position: a 16-mer further along the window
    # also lies in the copy before the window's own, so 23 copies can give 24 as well)
    w = _windows_of_class(gold, "in_t150_23")
    assert (gold.w["items"][w].max(1) == 23).any()


def test_reach_three_adjacent_rows_over_64(gold):
    it = gold.w["items"].astype(np.int64)
    three = it + np.roll(it, 1, 1) + np.roll(it, -1, 1)
    w = _windows_of_class(gold, "in_f3rows")
    assert (three[w] > 64).any()
    # and a slot of the middle row took votes after the three rows were full: it was found by the
    # second 64-lane pass of the scan (its place in the scan order row, row + 1, row - 1 is >= 64)
    assert (three[w] == 72).any()


def test_reach_more_than_64_used_slots(gold):
    for cls in ("in_r155_80", "id_r155_80", "in_f3rows"):
        w = _windows_of_class(gold, cls)
        assert (gold.w["n_used"][w] > 64).any(), cls


def test_reach_more_than_64_candidates(gold):
    votes = np.add.reduceat(np.concatenate([gold.s["votes"], [0]]).astype(np.int64), np.minimum(gold.first[:-1], len(gold.s)))
    votes[gold.w["n_used"] == 0] = 0
    for cls in ("in_t150_24", "in_r155_80", "in_f3rows"):
        w = _windows_of_class(gold, cls)
        assert (votes[w] > 64).any(), cls


def test_reach_border_drop(gold):
    """the index pads 1210 bases past the genome's last base, so on a one-block index the high border
    (block end - read length - window length) reaches back into the genome only for the longest
    reads, by 59 bases.  Only this high border is shown from the reference's tables: the low border
    and a border at a block boundary need the two-block index, which the golden does not hold; those
    are compared between the GPU and the restatement only (test_gpu_fragile.py, fredge_fullM1, classes
    blk1 / blkhigh / ov_s3 / ov_e2).  The 12-copy array edge_last at the genome's end shows the drop: window 0's
    top slots give the read's places in the array, P0 + start - 150 k are window w's; one of them
    that is past the border, but whose first subread still lies inside the genome, has no slot,
    while the copy before it has."""
    w = gold.w
    for cls in ("ov_last", "hi_last"):
        seen = 0
        idx = _windows_of_class(gold, cls)
        idx = idx[w["full_rl"][idx] == 1209]
        for c in np.unique(w["call"][idx]):
            win = idx[w["call"][idx] == c]
            t0 = gold.table(win[0])
            if w["max_vote"][win[0]] < 10:
                continue   # the other strand's call
            p0 = int(t0["pos"][t0["votes"] == w["max_vote"][win[0]]].max())
            for i in win[1:]:
                limit = int(w["high_border"][i]) - int(w["length"][i])
                genome_end = int(w["high_border"][i]) + 1209 - 1210
                t = gold.table(i)
                for k in range(12):
                    q = p0 + int(w["start"][i]) - 150 * k
                    if limit < q and q + 16 <= genome_end:
                        assert q not in t["pos"] and q - 150 in t["pos"]
                        seen += 1
        assert seen, cls


def test_reach_retry_set(index_cache):
    """the retry set reports more slots than svg_fragile_batch's first slot buffer holds
    (2 * windows + 1024, svg_fragile.hip)"""
    from oracle.pyoracle import OracleIndex
    from subread_amd.abi import default_params, PROGRAM_SUBJUNC
    w, s = OracleIndex(index_cache.get("fredge_full")).fragile(default_params(PROGRAM_SUBJUNC, False), fredge_retry_reads())
    assert len(s) > 2 * len(w) + 1024, (len(s), len(w))
    assert len(s) == int(w["n_slots"].sum())


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_oracle_equals_reference(name, index_cache):
    from oracle.pyoracle import OracleIndex
    g = fragile_golden(name)
    got = OracleIndex(index_cache.get(g.key)).fragile(g.params, g.reads.r1, g.reads.r2)
    assert_equals_reference(got, g)


def _layout(rl):
    """core-junction.c:5153-5180: windows and overlap at 5153-5154 (the division in double, stored in
    a float), window_cursor at 5177 (int * int - int * float: a float product and difference)"""
    windows = rl // 60 + 1
    overlap = np.float32((1.0 * windows * 60 - rl) / (windows - 1))
    out = []
    for ww in range(windows):
        cursor = int(np.float32(ww * 60) - np.float32(ww) * overlap)
        out.append((cursor, rl - cursor if ww == windows - 1 else 60))
    return out


def test_window_layout_every_length(index_cache):
    from oracle.pyoracle import OracleIndex
    from subread_amd.abi import ReadBatch, default_params, PROGRAM_SUBJUNC
    lens = list(range(161, 1210))
    rng = np.random.default_rng(5)
    reads = ReadBatch.from_list([np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes() for L in lens])
    w, _ = OracleIndex(index_cache.get("fredge_full")).fragile(default_params(PROGRAM_SUBJUNC, False), reads)
    w = w[w["strand"] == 0]
    for i, L in enumerate(lens):
        mine = w[w["read"] == i]
        assert [(int(a), int(b)) for a, b in zip(mine["start"], mine["length"])] == _layout(L), L


def test_window_layout_equals_reference_at_golden_lengths():
    g = fragile_golden("fredge_full_se")
    for L in FREDGE_LENGTHS:
        w = g.w[(g.w["full_rl"] == L)]
        first_call = w[w["call"] == w["call"][0]]
        assert [(int(a), int(b)) for a, b in zip(first_call["start"], first_call["length"])] == _layout(L), L
        assert len(set(zip(w["window"].tolist(), w["start"].tolist(), w["length"].tolist()))) == len(first_call)
