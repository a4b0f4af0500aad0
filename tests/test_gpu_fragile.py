"""GPU: fragile junction voting of subjunc reads > 160 bp (svg_fragile_batch, svg_fragile.hip;
core_fragile_junction_voting, core-junction.c:5151-5422) -- every window record (junction
split and sides, GT/AG strand) and every reported top-vote slot (position, indel recorder)
byte-identical to the CPU restatement (oracle/svoracle.c svo_fragile_batch), whose events are
pinned to the reference's own event tables in tests/test_events.py:
  * the golden long subjunc cases (full, gapped and 4-block indexes, SE and PE);
  * simulated spliced reads of 161-1209 bases on full / gapped / multi-block indexes, SE and PE,
    with mismatches, indels and N bases;
  * the fredge read classes (tests/common.py: full rows, three full neighbouring rows, more than 64
    used slots and candidates, borders, contig ends, N / lowercase / IUPAC / U) -- against the
    REFERENCE's own dumped window tables (tests/golden/fragile, tests/fragile_common.py) and, in
    larger draws on one- and two-block indexes, against the restatement;
  * a batch that reports more slots than the first slot buffer holds (the host's retry);
  * a batch mixing short, empty and long reads.
The reference-event check of the GPU windows themselves is test_events.py's GPU test."""
import numpy as np
import pytest

from tests.common import Case, FREDGE_LENGTHS, ensure_built, fredge_reads, fredge_retry_reads
from tests.fragile_common import GOLDEN_SETS, assert_equals_reference, fragile_golden

ensure_built()
pytestmark = pytest.mark.gpu

LONG_CASES = ["sj_se_full_long", "sj_pe_gapped_long", "sj_se_mb_synth_long_fullM1"]


def _same(got, want):
    (gw, gs), (ww, ws) = got, want
    assert len(gw) == len(ww), (len(gw), len(ww))
    bad = np.nonzero(gw.view(np.uint8).reshape(len(gw), -1) != ww.view(np.uint8).reshape(len(ww), -1))[0]
    assert not len(bad), "%d windows differ, first: gpu %s / cpu %s" % (len(set(bad)), gw[bad[0]], ww[bad[0]])
    assert len(gs) == len(ws), (len(gs), len(ws))
    assert (gs.view(np.uint8) == ws.view(np.uint8)).all(), "reported slots differ"


@pytest.mark.parametrize("name", LONG_CASES)
def test_fragile_windows_golden_cases(name, index_cache):
    import subread_amd as sa
    from oracle.pyoracle import OracleIndex
    c = Case(name)
    pre = index_cache.get(c.index_key)
    ix = sa.VoteIndex(pre, device=0)
    got = ix.fragile(c.params, c.r1, c.r2)
    ix.close()
    want = OracleIndex(pre).fragile(c.params, c.r1, c.r2)
    _same(got, want)
    assert got[0]["junction"].sum() > 0


def _spliced(g, n, lens, seed):
    from subread_amd.abi import ReadBatch
    from subread_amd.sim import simulate_spliced_reads
    parts = [simulate_spliced_reads(g, n, L, seed=seed + L, max_intron=20000) for L in lens]
    reads = [b.read(i) for b in parts for i in range(len(b))]
    rng = np.random.default_rng(seed)
    out = []
    for r in reads:   # sprinkle N and a few 1-3 base indels
        r = bytearray(r)
        if rng.random() < 0.2:
            at = int(rng.integers(20, len(r) - 20))
            if rng.random() < 0.5:
                del r[at:at + int(rng.integers(1, 4))]
            else:
                r[at:at] = bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 4))))
        for i in rng.choice(len(r), int(rng.integers(0, 3)), replace=False):
            r[int(i)] = ord("N")
        out.append(bytes(r))
    return ReadBatch.from_list(out)


@pytest.mark.parametrize("probe", ["image", "literal"])
@pytest.mark.parametrize("key,paired", [("chr901_full", False), ("chr901_gapped", True), ("long777_gappedM6", False),
                                        ("synth4242_fullM1", True)])
def test_fragile_windows_simulated(key, paired, probe, index_cache, svgopt):
    """probe: the equal-key runs from the probe images (bucket code / key-hash, go_run) or the literal
    gehash_go_q search (option keys_literal) -- identical windows either way"""
    import subread_amd as sa
    from oracle.pyoracle import OracleIndex
    from subread_amd.abi import default_params, PROGRAM_SUBJUNC
    from subread_amd.sim import Genome
    pre = index_cache.get(key)
    g = Genome.read_fasta(index_cache.genome_fasta(key.rsplit("_", 1)[0]))
    lens = (161, 200, 257, 400, 700, 1209)
    r1 = _spliced(g, 150, lens, 71)
    r2 = _spliced(g, 150, lens, 83) if paired else None
    p = default_params(PROGRAM_SUBJUNC, paired)
    svgopt.set("keys_literal", 1 if probe == "literal" else 0)
    ix = sa.VoteIndex(pre, device=0)
    got = ix.fragile(p, r1, r2)
    ix.close()
    want = OracleIndex(pre).fragile(p, r1, r2)
    _same(got, want)
    assert want[0]["junction"].sum() > 0


@pytest.mark.parametrize("probe", ["image", "literal"])
@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_fragile_windows_equal_reference_tables(name, probe, index_cache, svgopt):
    """the GPU's windows and reported slots against the reference's own dump, directly"""
    import subread_amd as sa
    g = fragile_golden(name)
    svgopt.set("keys_literal", 1 if probe == "literal" else 0)
    ix = sa.VoteIndex(index_cache.get(g.key), device=0)
    got = ix.fragile(g.params, g.reads.r1, g.reads.r2)
    ix.close()
    assert_equals_reference(got, g)


def _tiles(w, n_slots):
    """every block's first_slot ranges tile the slot list without gap or overlap, in window order"""
    at = 0
    for b in np.unique(w["block"]):
        wb = w[w["block"] == b]
        first = at + np.concatenate([[0], np.cumsum(wb["n_slots"].astype(np.int64))])
        assert (wb["first_slot"][wb["n_slots"] > 0] == first[:-1][wb["n_slots"] > 0]).all(), "block %d" % b
        at = int(first[-1])
    assert at == n_slots


@pytest.mark.parametrize("key,paired", [("fredge_full", False), ("fredge_full", True), ("fredge_gapped", False),
                                        ("fredge_gapped", True), ("fredge_fullM1", False), ("fredge_fullM1", True)])
def test_fragile_fredge_classes(key, paired, index_cache):
    """larger seeded draws of every fredge class: 49 reads per class at the seven lengths up to 241
    and 4 at 700 and 1209 bases"""
    import subread_amd as sa
    from oracle.pyoracle import OracleIndex
    from subread_amd.abi import default_params, PROGRAM_SUBJUNC
    pre = index_cache.get(key)
    p = default_params(PROGRAM_SUBJUNC, paired)
    ix = sa.VoteIndex(pre, device=0)
    oi = OracleIndex(pre)
    for per, lens, seed in ((7, FREDGE_LENGTHS[:7], 211), (2, FREDGE_LENGTHS[7:], 223)):
        r = fredge_reads(per, seed + paired, lengths=lens, paired=paired)
        got = ix.fragile(p, r.r1, r.r2)
        want = oi.fragile(p, r.r1, r.r2)
        _same(got, want)
        assert want[0]["junction"].sum() > 0 and len(want[1]) > 0
        _tiles(got[0], len(got[1]))
        assert len(np.unique(got[0]["block"])) == (2 if key.endswith("M1") else 1)
    ix.close()


def test_fragile_slot_buffer_retry(index_cache):
    """more reported slots than the first slot buffer (2 * windows + 1024) holds: the second
    attempt's result is complete and in window order, and leaves no state behind"""
    import subread_amd as sa
    from oracle.pyoracle import OracleIndex
    from subread_amd.abi import default_params, PROGRAM_SUBJUNC
    pre = index_cache.get("fredge_full")
    p = default_params(PROGRAM_SUBJUNC, False)
    big = fredge_retry_reads()
    small = fredge_reads(1, 5, lengths=(161, 240)).r1
    want, want_small = OracleIndex(pre).fragile(p, big), OracleIndex(pre).fragile(p, small)
    assert len(want[1]) > 2 * len(want[0]) + 1024
    ix = sa.VoteIndex(pre, device=0)
    got = ix.fragile(p, big)
    after = ix.fragile(p, small)
    again = ix.fragile(p, big)
    ix.close()
    _same(got, want)
    assert len(got[1]) == int(got[0]["n_slots"].sum())
    _tiles(got[0], len(got[1]))
    _same(after, want_small)
    _same(again, want)


def test_fragile_mixed_batch(index_cache):
    """reads of 160 bases or fewer, empty reads and reads over 160 bases in one paired batch: only
    the long ends give windows, and `read` is the read's number in the batch"""
    import subread_amd as sa
    from oracle.pyoracle import OracleIndex
    from subread_amd.abi import ReadBatch, default_params, PROGRAM_SUBJUNC
    pre = index_cache.get("fredge_gapped")
    p = default_params(PROGRAM_SUBJUNC, True)
    src = fredge_reads(1, 9, lengths=(161, 241), paired=True)
    rng = np.random.default_rng(3)
    a, b = [], []
    for i in range(len(src.r1)):
        x, y = src.r1.read(i), src.r2.read(i)
        k = int(rng.integers(0, 6))
        a.append(x if k in (0, 1) else x[:int(rng.integers(16, 161))] if k in (2, 3) else b"" if k == 4 else x[:160])
        b.append(y if k in (0, 2) else y[:int(rng.integers(16, 161))] if k in (1, 3) else b"" if k == 5 else y[:160])
    r1, r2 = ReadBatch.from_list(a), ReadBatch.from_list(b)
    ix = sa.VoteIndex(pre, device=0)
    got = ix.fragile(p, r1, r2)
    ix.close()
    _same(got, OracleIndex(pre).fragile(p, r1, r2))
    w = got[0]
    long_ends = {(i, e) for e, rb in enumerate((r1, r2)) for i in range(len(rb)) if rb.lens[i] > 160}
    assert {(int(r), int(e)) for r, e in zip(w["read"], w["end"])} == long_ends and len(long_ends) > 10
    for e, rb in enumerate((r1, r2)):
        sel = w[(w["end"] == e) & (w["strand"] == 0) & (w["window"] == 0)]
        assert (sel["read"][1:] > sel["read"][:-1]).all()
        last = w[(w["end"] == e) & (w["strand"] == 0)]
        assert (last["start"].astype(np.int64) + last["length"] <= rb.lens[last["read"]]).all()
