"""GPU: the line probe kernel's per-read plan and slot-major read groups (svg_plan.h) leave
every record as it was -- byte-identical to the oracle on one small genome with repeat families,
at the shapes where the grouping can go wrong: partial and exact groups, a block without a group,
read lengths around every threshold mixed in one batch (no probe below 15 + gap, the lane / SoA
path up to 160, the wave / AoS path above; a 200-base bound makes the group a power of two below
64), single-end, -S and pairs with different R1 / R2 lengths, ASCII and packed input with an
exception mask, gap 1 and gap 3 indexes and every probe image."""
import numpy as np
import pytest

from tests.common import ensure_built, pack_records, describe_mismatch

ensure_built()
pytestmark = pytest.mark.gpu

LENS_SHORT = [15, 16, 17, 18, 31, 99, 100, 159, 160]      # bound 160: lane kernels, SoA records
LENS_LONG = LENS_SHORT + [161, 200]                         # bound 200: wave kernel, AoS records
COUNTS = [1, 63, 64, 65, 129]


def _truncate(rb, lens):
    """reads of 200 bases cut to the lengths of `lens`, cycled (the text keeps its 200-base pitch)"""
    from subread_amd.abi import ReadBatch
    n = len(rb)
    return ReadBatch(rb.seq, rb.offsets, np.resize(np.array(lens, np.uint16), n))


@pytest.fixture(scope="module")
def world():
    """genome, reads (n = 64 x CUs + 1: with one block per CU some blocks get no group) and the
    oracle's records and statistics per (gap, mode, length set), computed once"""
    import torch
    import subread_amd as sa
    from oracle.pyoracle import OracleIndex
    from subread_amd.abi import default_params, PROGRAM_ALIGN
    from subread_amd.sim import random_genome, simulate_reads
    g = random_genome([1_000_000], 91, repeats=(3000, 300, 6, 0.05))
    n = 64 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    raw1 = simulate_reads(g, n, 200, seed=7, sub=0.01, indel=0.002, nrate=0.004)
    raw2 = simulate_reads(g, n, 200, seed=8, sub=0.01, indel=0.002, nrate=0.004)
    reads = {}
    for name, lens in (("short", LENS_SHORT), ("long", LENS_LONG)):
        reads[name] = (_truncate(raw1, lens), _truncate(raw2, lens[::-1]))   # a pair's ends differ in length
    arrays, refs = {}, {}

    def params(mode):
        p = default_params(PROGRAM_ALIGN, mode == "pe")
        if mode == "rev":
            p.reverse_r1 = 1
        return p

    def ref(gap, mode, lset):
        k = (gap, mode, lset)
        if k not in refs:
            if gap not in arrays:
                ix = sa.VoteIndex.build_genome(g, gap=gap, force_one_block=True, repeat_threshold=400, device=0)
                arrays[gap] = ix.export()
                ix.close()
            r1, r2 = reads[lset]
            out, _, _, st = OracleIndex(arrays=arrays[gap]).vote(params(mode), r1, r2 if mode == "pe" else None, threads=16)
            refs[k] = (pack_records(out, None, None), st)
        return refs[k]

    class W:
        pass
    w = W()
    w.g, w.n, w.reads, w.params, w.ref, w.arrays = g, n, reads, params, ref, arrays
    return w


def _vote(ix, w, mode, lset, n, packed):
    import subread_amd as sa
    r1, r2 = w.reads[lset]
    r1, r2 = r1.slice(0, n), (r2.slice(0, n) if mode == "pe" else None)
    p = w.params(mode)
    if packed:
        # back to back (per-read starts); each end's own lengths
        k1 = sa.pack_reads(r1)
        k2 = sa.pack_reads(r2) if r2 is not None else None
        if n > 1000:
            assert k1.xmask is not None   # reads with N: the exception mask
        out, _, _ = ix.vote_packed(p, k1, k2)
    else:
        out, _, _ = ix.vote(p, r1, r2)
    return pack_records(out, None, None)


def _check(ix, w, gap, mode, lset, packed, svgopt, counts=None):
    want, _ = w.ref(gap, mode, lset)
    ends = 2 if mode == "pe" else 1
    for n in (counts or COUNTS):
        got = _vote(ix, w, mode, lset, n, packed)
        assert (got == want[:n]).all(), "n %d: %s" % (n, describe_mismatch(got, want[:n], ends, 3))
    # one block per CU: ceil(groups / blocks) groups per block leave the last blocks without any
    svgopt.set("probe_cap", 1)
    got = _vote(ix, w, mode, lset, w.n, packed)
    svgopt.reset("probe_cap")
    assert (got == want).all(), "n %d: %s" % (w.n, describe_mismatch(got, want, ends, 3))


@pytest.fixture(scope="module")
def full_index(world):
    import subread_amd as sa
    ix = sa.VoteIndex.build_genome(world.g, gap=1, force_one_block=True, repeat_threshold=400, device=0)
    yield ix
    ix.close()


@pytest.mark.parametrize("packed", [False, True], ids=["ascii", "packed"])
@pytest.mark.parametrize("lset", ["short", "long"])
@pytest.mark.parametrize("mode", ["se", "rev", "pe"])
def test_gpu_plan_code_image_matches_oracle(mode, lset, packed, world, full_index, svgopt):
    """the default image of a full index (32-byte bucket codes)"""
    _check(full_index, world, 1, mode, lset, packed, svgopt)
    sizes = np.diff(world.arrays[1]["bstart"].astype(np.int64))
    assert (sizes > 59).sum() > 0   # the repeat families make big buckets


@pytest.mark.parametrize("env", [{"no_bcode": 1}, {"no_bcode": 1, "no_khash": 1}, {"no_compact": 1}],
                         ids=["khash", "line", "plain"])
@pytest.mark.parametrize("gap", [1, 3])
def test_gpu_plan_images_match_oracle(gap, env, world, svgopt):
    """gap 1 and gap 3 indexes with each probe image forced (a gap 3 index has the key-hash image
    by default)"""
    import subread_amd as sa
    for k, v in env.items():
        svgopt.set(k, v)
    ix = sa.VoteIndex.build_genome(world.g, gap=gap, force_one_block=True, repeat_threshold=400, device=0)
    for k in env:
        svgopt.reset(k)
    try:
        for mode, lset, packed in (("se", "short", True), ("pe", "short", False), ("se", "long", False), ("pe", "long", True)):
            _check(ix, world, gap, mode, lset, packed, svgopt, counts=[1, 65])
    finally:
        ix.close()


@pytest.mark.parametrize("env", [{}, {"no_bcode": 1}, {"no_bcode": 1, "no_khash": 1}], ids=["code", "khash", "line"])
def test_gpu_plan_statistics_match_oracle(env, world, svgopt):
    """probes / bucket_items / hits with statistics on equal the oracle's counts (the counters are
    kept only when asked for)"""
    import subread_amd as sa
    for k, v in env.items():
        svgopt.set(k, v)
    ix = sa.VoteIndex.build_genome(world.g, gap=1, force_one_block=True, repeat_threshold=400, device=0)
    for k in env:
        svgopt.reset(k)
    try:
        for mode, lset in (("se", "short"), ("pe", "long")):
            want, st = world.ref(1, mode, lset)
            ix.set_stats(True)
            got = _vote(ix, world, mode, lset, world.n, True)
            s = ix.stats()
            ix.set_stats(False)
            print(mode, lset, env, s, [int(x) for x in st])
            assert (got == want).all()
            assert (s["probes"], s["bucket_items"], s["hits"]) == (int(st[0]), int(st[1]), int(st[2]))
    finally:
        ix.close()
