"""GPU: the count bins of the fused single-end lane path (svg_lane.hip, lane_bin_kernel and
lane_kernel's group lookup) under both rules of option lane_bins -- 0: lists by heavier strand and
its count class; 1: one list per class of the
larger strand count.  A rule only decides which reads share a wave: records, deferrals and the
deferral reasons must not depend on it, at every batch size where a group, a tile or a list ends
part-filled, with lists empty, and in subjunc mode.  The step counter (word 28 of debug_counters)
shows that the new rule does what it is for."""
import numpy as np
import pytest

from tests.common import Case, ensure_built, pack_records, describe_mismatch, vtedge_se_reads

ensure_built()
pytestmark = pytest.mark.gpu

RULES = [0, 1]
N_MAX = 8200   # eight 1024-read tiles and a bit


@pytest.fixture(scope="module")
def gpu_indexes(index_cache):
    import subread_amd as sa
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = sa.VoteIndex(index_cache.get(key), device=0)
        return cache[key]
    yield get
    for v in cache.values():
        v.close()


@pytest.fixture(scope="module")
def chr901(index_cache):
    """N_MAX chr901 reads in random orientation with substitutions, indels and Ns, their strands,
    and their oracle records (made once; a read's records do not depend on its batch)"""
    from oracle.pyoracle import OracleIndex
    from subread_amd.abi import default_params, PROGRAM_ALIGN
    from subread_amd.sim import Genome, simulate_reads
    g = Genome.read_fasta(index_cache.genome_fasta("chr901"))
    rb, _, _, strand = simulate_reads(g, N_MAX, 100, seed=977, sub=0.02, indel=0.02, nrate=0.002, truth=True)
    p = default_params(PROGRAM_ALIGN, False)
    ref, _, _, _ = OracleIndex(index_cache.get("chr901_full")).vote(p, rb, threads=16)
    return p, rb, strand, pack_records(ref, None, None)


def vote_with_counters(ix, p, rb, svgopt, rule, **opts):
    svgopt.set("lane_bins", rule)
    for k, v in opts.items():
        svgopt.set(k, v)
    ix.set_stats(True)
    try:
        out, jout, bm = ix.vote(p, rb)
        st, dc = ix.stats(), [int(x) for x in ix.debug_counters()]
    finally:
        ix.set_stats(False)
    return out, jout, bm, st, dc


def subset(rb, idx):
    from subread_amd.abi import ReadBatch
    return ReadBatch.from_list([rb.read(int(i)) for i in idx])


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 4095, 4096, 4097, N_MAX])
def test_group_tile_and_list_edges_match_oracle(n, rule, gpu_indexes, chr901, svgopt):
    p, rb, _, want = chr901
    svgopt.set("lane_bins", rule)
    out, _, _ = gpu_indexes("chr901_full").vote(p, rb.slice(0, n))
    got = pack_records(out, None, None)
    assert (got == want[:n]).all(), describe_mismatch(got, want[:n], 1, 3)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("which", ["forward", "reverse", "nohit", "deferred"])
def test_empty_lists(which, rule, gpu_indexes, chr901, index_cache, svgopt):
    """One orientation's lists empty; only reads without a hit on either strand (one list); every
    read deferred (option lane 2: every list empty)."""
    from oracle.pyoracle import OracleIndex
    from subread_amd.abi import ReadBatch
    p, rb, strand, want = chr901
    ix = gpu_indexes("chr901_full")
    if which == "nohit":
        rng = np.random.default_rng(11)
        sub = ReadBatch.fixed(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (1500, 100))])
        ref, _, _, _ = OracleIndex(index_cache.get("chr901_full")).vote(p, sub, threads=16)
        w = pack_records(ref, None, None)
    else:
        idx = np.arange(1500) if which == "deferred" else np.flatnonzero(strand == (which == "reverse"))[:1500]
        assert len(idx) == 1500
        sub, w = subset(rb, idx), want[idx]
    out, _, _, st, dc = vote_with_counters(ix, p, sub, svgopt, rule, lane=2 if which == "deferred" else 1)
    got = pack_records(out, None, None)
    assert (got == w).all(), describe_mismatch(got, w, 1, 3)
    if which == "deferred":
        assert st["deferred"] == 1500 and dc[28] == 0
    if which == "nohit":
        assert st["deferred"] == 0 and dc[19] < 100   # a handful of chance hits on 1 Mbp


@pytest.mark.parametrize("case", ["vtedge", "chr901"])
def test_same_deferrals_under_both_rules(case, gpu_indexes, chr901, index_cache, svgopt):
    from oracle.pyoracle import OracleIndex
    if case == "vtedge":
        from subread_amd.abi import default_params, PROGRAM_ALIGN
        v = vtedge_se_reads(60, 206)
        p, rb, key = default_params(PROGRAM_ALIGN, False), v.r1, "vtedge_full"
        ref, _, _, _ = OracleIndex(index_cache.get(key)).vote(p, rb, threads=16)
        want = pack_records(ref, None, None)
    else:
        p, rb, _, want = chr901
        key = "chr901_full"
    res = [vote_with_counters(gpu_indexes(key), p, rb, svgopt, rule, lane=1) for rule in RULES]
    for out, _, _, st, dc in res:
        got = pack_records(out, None, None)
        assert (got == want).all(), describe_mismatch(got, want, 1, 3)
    (_, _, _, st0, dc0), (_, _, _, st1, dc1) = res
    assert st0["deferred"] == st1["deferred"]
    assert case != "vtedge" or st0["deferred"] > 0   # the ladder classes past the limits
    assert dc0[16:21] == dc1[16:21]
    assert st0 == st1


@pytest.mark.parametrize("rule", RULES)
def test_subjunc_golden(rule, gpu_indexes, svgopt):
    c = Case("sj_se_full_vtedge")
    svgopt.set("lane_bins", rule)
    svgopt.set("lane", 1)
    out, jout, bm = gpu_indexes(c.index_key).vote(c.params, c.r1, c.r2)
    got = pack_records(out, jout, bm)
    assert (got == c.expected).all(), describe_mismatch(got, c.expected, c.ends, c.params.multi_best)


def test_strand_rule_runs_fewer_vote_steps(gpu_indexes, chr901, svgopt, capsys):
    """On the 1 Mbp genome a read's hits are nearly all on its own strand: grouping by the larger
    count alone makes every wave run both strands' loops to the top; by strand it does not."""
    p, rb, strand, _ = chr901
    assert 0.4 < strand.mean() < 0.6
    ix = gpu_indexes("chr901_full")
    dc = [vote_with_counters(ix, p, rb, svgopt, rule, lane=1)[4] for rule in RULES]
    with capsys.disabled():
        print("\nlane_bins 0 / 1: vote-loop steps %d / %d, tail steps %d / %d, candidates %d" % (
            dc[0][28], dc[1][28], dc[0][29], dc[1][29], dc[0][19]))
    assert dc[0][19] == dc[1][19] > 0
    assert 0 < dc[0][28] < dc[1][28]
    assert dc[0][19] <= 64 * dc[0][28]     # utilisation <= 1
