"""GPU: the vtedge read classes (tests/common.py: full vote-table rows, tandem and row-rotating
arrays, microsatellites, the lane kernels' candidate / slot limits at N and N + 1, reads hanging
over the genome's ends) in larger numbers than the reference-made goldens hold, against the oracle
restatement byte for byte, through what the goldens cannot vary: packed input, the device entry,
the host and chunk pipelines, a multi-block index and every probe image.  tests/test_vtedge.py
shows from the sequences alone that the classes reach those edges; the *_vtedge goldens pin the
oracle to the reference's own records on them."""
import numpy as np
import pytest

from tests.common import (ensure_built, pack_records, describe_mismatch, vtedge_layout, vtedge_se_reads,
                          vtedge_pe_reads, vtedge_sj_reads)

ensure_built()
pytestmark = pytest.mark.gpu


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
def sets(index_cache):
    """read sets and their oracle records, made once: sets(mode, key) -> (params, r1, r2, want, reads)"""
    from oracle.pyoracle import OracleIndex
    from subread_amd.abi import default_params, PROGRAM_ALIGN, PROGRAM_SUBJUNC
    reads, cache = {}, {}

    def get(mode, key):
        if (mode, key) in cache:
            return cache[mode, key]
        gapped = key.rsplit("_", 1)[1].startswith("gapped")
        rk = (mode, gapped and mode == "se")
        if rk not in reads:
            if mode == "se":        # ~20,000 reads of <= 160 bp (the lane kernels' batches)
                reads[rk] = vtedge_se_reads(350, 201, ladder=(18, 19, 20, 21) if gapped else (16, 17, 18, 19))
            elif mode == "se161":   # a batch with 161-bp reads: wave kernel, long-read subread step
                reads[rk] = vtedge_se_reads(60, 204, with_161=True)
            elif mode == "pe":      # ~3,000 pairs
                reads[rk] = vtedge_pe_reads(270, 202)
            elif mode == "sj":      # ~1,500 spliced 100-bp reads (the subjunc lane kernel's batch)
                reads[rk] = vtedge_sj_reads(125, 203, lengths=(100,))
            else:                   # with 200-bp reads
                reads[rk] = vtedge_sj_reads(60, 205)
        v = reads[rk]
        sj = mode.startswith("sj")
        p = default_params(PROGRAM_SUBJUNC if sj else PROGRAM_ALIGN, mode == "pe")
        ref, rj, rbm, _ = OracleIndex(index_cache.get(key)).vote(p, v.r1, v.r2, threads=16)
        cache[mode, key] = (p, v.r1, v.r2, pack_records(ref, rj if sj else None, rbm if sj else None), v)
        return cache[mode, key]
    return get


def same(got, want, ends, what=""):
    assert (got == want).all(), "%s: %s" % (what, describe_mismatch(got, want, ends, 3))


@pytest.mark.parametrize("mode,key", [("se", "vtedge_full"), ("se", "vtedge_gapped"), ("se161", "vtedge_full"),
                                      ("pe", "vtedge_full"), ("pe", "vtedge_gapped"), ("sj", "vtedge_full"),
                                      ("sj200", "vtedge_full"), ("sj", "vtedge_gapped")])
def test_gpu_vtedge_entries_match_oracle(mode, key, gpu_indexes, sets):
    """ASCII and packed host input and (align mode) the device entry."""
    import subread_amd as sa
    import torch
    p, r1, r2, want, _ = sets(mode, key)
    ix = gpu_indexes(key)
    sj = mode.startswith("sj")
    ends = 2 if r2 is not None else 1
    out, jout, bm = ix.vote(p, r1, r2)
    same(pack_records(out, jout if sj else None, bm if sj else None), want, ends, "ascii")
    out, jout, bm = ix.vote_packed(p, sa.pack_reads(r1, None), sa.pack_reads(r2, None) if r2 is not None else None)
    same(pack_records(out, jout if sj else None, bm if sj else None), want, ends, "packed")
    if not sj:
        dev = torch.device("cuda", 0)
        keep = []

        def dr(b):
            t = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev) for x in (b.seq, b.offsets, b.lens)]
            keep.append(t)
            return (t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(b))
        d_out = torch.zeros(len(r1) * ends * p.multi_best * 68, dtype=torch.uint8, device=dev)
        ix.vote_device(p, dr(r1), dr(r2) if r2 is not None else None, d_out.data_ptr())
        ix.device_status()
        same(d_out.cpu().numpy().reshape(len(r1), -1), want, ends, "device")


@pytest.mark.parametrize("mode", ["se", "pe", "sj"])
def test_gpu_vtedge_pipelines_match_oracle(mode, gpu_indexes, sets, svgopt):
    """Host sub-batches and probe-record chunks with ragged tails (as test_gpu_pipelines_match_oracle)."""
    p, r1, r2, want, _ = sets(mode, "vtedge_full")
    ix = gpu_indexes("vtedge_full")
    sj = mode == "sj"
    n = len(r1)
    for env in ({"host_sub": n // 3 + 7}, {"chunk": n // 7 + 3, "overlap": 1},
                {"host_sub": n // 2 + 5, "chunk": n // 9 + 1, "overlap": 1}):
        for k, v in env.items():
            svgopt.set(k, v)
        out, jout, bm = ix.vote(p, r1, r2)
        for k in env:
            svgopt.reset(k)
        same(pack_records(out, jout if sj else None, bm if sj else None), want, 2 if mode == "pe" else 1, str(env))


@pytest.mark.parametrize("mode", ["se", "pe", "sj"])
def test_gpu_vtedge_multi_block_matches_oracle(mode, sets, tmp_path_factory):
    """-F -M 1 splits the genome into 2 blocks: later blocks merge into the records left by a block in
    which a row was full."""
    import subread_amd as sa
    from oracle.pyoracle import OracleIndex
    from tests.common import synth_genome
    d = tmp_path_factory.mktemp("vtedge_mb")
    fa, pre = str(d / "vtedge.fa"), str(d / "idx")
    synth_genome("vtedge").write_fasta(fa)
    sa.build_index(fa, pre, gap=1, memory_mb=1, force_one_block=False)
    p, r1, r2, _, _ = sets(mode, "vtedge_full")
    sj = mode == "sj"
    ix = sa.VoteIndex(pre, device=0)
    try:
        assert ix.n_blocks > 1
        out, jout, bm = ix.vote(p, r1, r2)
    finally:
        ix.close()
    ref, rj, rbm, _ = OracleIndex(pre).vote(p, r1, r2, threads=16)
    same(pack_records(out, jout if sj else None, bm if sj else None),
         pack_records(ref, rj if sj else None, rbm if sj else None), 2 if mode == "pe" else 1)


def test_gpu_vtedge_probe_images_match_oracle(sets, svgopt):
    """Every probe image of test_gpu_probe_images_match_oracle on the vtedge index: the images
    differ in how an equal-key run is found, and a full row shows any change of its order."""
    import subread_amd as sa
    p, r1, _, want, _ = sets("se", "vtedge_full")
    g = vtedge_layout()[0]
    for env in ({}, {"no_bcode": 1}, {"no_bcode": 1, "khash64": 1}, {"no_bcode": 1, "no_khash": 1},
                {"no_bcode": 1, "no_khash": 1, "no_bline": 1}, {"no_compact": 1}):
        for k, v in env.items():
            svgopt.set(k, v)
        ix = sa.VoteIndex.build_genome(g, gap=1, force_one_block=True, device=0)
        for k in env:
            svgopt.reset(k)
        try:
            out, _, _ = ix.vote(p, r1)
        finally:
            ix.close()
        same(pack_records(out, None, None), want, 1, str(env))


@pytest.mark.parametrize("unfused,cls,deferred", [
    (0, "lad16_16", 0), (0, "lad17_16", 0), (0, "lad16_17", 1), (0, "lad17_17", 1), (0, "lad18_15", 1),
    (0, "lad18_16", 1), (0, "lad17_20", 1), (0, "lad16_21", 1), (0, "lad17_21", 1), (0, "lad18_21", 1),
    (0, "lad19_21", 1),
    (1, "lad16_20", 0), (1, "lad17_20", 0), (1, "lad16_21", 1), (1, "lad17_21", 1), (1, "lad17_19", 0),
    (1, "lad18_15", 1), (1, "lad18_19", 1)])
def test_gpu_vtedge_lane_limits_are_exact(unfused, cls, deferred, gpu_indexes, sets, svgopt):
    """Single-end align on the full index keeps a read on the lane kernel while each strand has at
    most LANE_CAP1 = 40 candidates and the read at most LANE_K1 = 16 slots (20, LANE_K1_WIDE, with
    the separate gather kernel, option lane_unfused; svg_lane.hip).  A lad<L>_<n> read has
    (L - 15) * n candidates and n slots on one strand, none on the other (tests/test_vtedge.py),
    and no indel, so no other reason to defer.
    Fused, 16 slots: the 16- and 17-bp reads of the 16-copy array (16 and 32 candidates, 16 slots)
    all stay; its 18-bp reads (48 candidates) and the 15-copy array's (45) are all deferred; 17
    copies are one slot too many; 20 and 21 copies are deferred at every length.
    Unfused, 20 slots: there the candidate limit decides alone.  17-bp reads on 20 copies have
    exactly 40 candidates and 20 slots and all stay, on 21 copies 42 and 21 and all are deferred;
    18-bp reads on 15 and 19 copies (45, 57 candidates, slots within 20) are deferred by the
    candidate limit only; 16-bp reads on 21 copies (21 candidates) by the slot limit only."""
    p, r1, r2, want, v = sets("se", "vtedge_full")
    keep = v.cls == cls
    n = int(keep.sum())
    assert n >= 30
    sub = v.select(keep)
    ix = gpu_indexes("vtedge_full")
    svgopt.set("lane", 1)
    svgopt.set("lane_unfused", unfused)
    ix.set_stats(True)
    try:
        out, _, _ = ix.vote(p, sub.r1)
        st = ix.stats()
    finally:
        ix.set_stats(False)
    same(pack_records(out, None, None), want[keep], 1, cls)
    assert st["deferred"] == (n if deferred else 0), (cls, st)
