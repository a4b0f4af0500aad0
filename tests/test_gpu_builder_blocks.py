"""GPU index builder, multi-block: svg_index_build* makes the reference's block structure in HBM
(kept bitmap + block plan, one table per block), its files are md5-identical to
subread-buildindex -M n, and the handle votes the golden multi-block records."""
import glob
import os

import numpy as np
import pytest

from tests.common import (Case, describe_mismatch, ensure_built, index_md5, index_recipe, is_multi_block_key, md5,
                          pack_records)

ensure_built()
pytestmark = pytest.mark.gpu

MB_KEYS = sorted(k for k in index_md5()["md5"] if is_multi_block_key(k))
MB_CASES = ["se_mb_synth_fullM1", "pe_mb_synth_gappedM1", "pe_mb_long_fullM17", "se_mb_long_gappedM6",
            "se_mb_vtedge_fullM1", "sj_se_mb_synth_fullM1", "sj_se_mb_synth_long_fullM1", "sj_pe_mb_long_gappedM6"]


def fixture_blocks(key):
    return sum(1 for suf in index_md5()["md5"][key] if suf.endswith(".b.tab"))


def block_files(pre):
    return sorted(os.path.basename(p)[len(os.path.basename(pre)):] for p in glob.glob(pre + ".[0-9][0-9].b.*"))


@pytest.fixture(scope="module")
def saved_builds(index_cache, tmp_path_factory):
    """key -> (handle built in HBM with its files saved, prefix); a stale block 09 lay there before"""
    import subread_amd as sa
    root = tmp_path_factory.mktemp("gpu_blocks")
    cache = {}

    def get(key):
        if key not in cache:
            gname, gap, memory_mb, force = index_recipe(key)
            pre = str(root / key)
            for suf in (".09.b.tab", ".09.b.array"):
                with open(pre + suf, "wb") as f:
                    f.write(b"stale")
            ix = sa.VoteIndex.build(index_cache.genome_fasta(gname), gap=gap, memory_mb=memory_mb, force_one_block=force,
                                    device=0, save_prefix=pre)
            cache[key] = (ix, pre)
        return cache[key]
    yield get
    for ix, _ in cache.values():
        ix.close()


@pytest.fixture(scope="module")
def hbm_builds(index_cache):
    """key -> handle built in HBM, nothing written"""
    import subread_amd as sa
    cache = {}

    def get(key):
        if key not in cache:
            gname, gap, memory_mb, force = index_recipe(key)
            cache[key] = sa.VoteIndex.build(index_cache.genome_fasta(gname), gap=gap, memory_mb=memory_mb,
                                            force_one_block=force, device=0)
        return cache[key]
    yield get
    for ix in cache.values():
        ix.close()


def test_fixture_keys():
    assert MB_KEYS == sorted(["synth4242_fullM1", "synth4242_gappedM1", "long777_fullM17", "long777_gappedM6", "vtedge_fullM1",
                              "fredge_fullM1"])
    assert [fixture_blocks(k) for k in ("synth4242_fullM1", "synth4242_gappedM1", "long777_fullM17", "long777_gappedM6",
                                        "vtedge_fullM1", "fredge_fullM1")] == [4, 2, 6, 4, 2, 2]


@pytest.mark.parametrize("key", MB_KEYS)
def test_gpu_built_blocks_md5(key, saved_builds):
    ix, pre = saved_builds(key)
    want = index_md5()["md5"][key]
    assert not index_recipe(key)[3]
    assert ix.n_blocks == fixture_blocks(key)
    for suf, m in want.items():
        assert md5(pre + suf) == m, (key, suf)
    # nothing beyond the last block: the stale block 09 is gone
    assert block_files(pre) == sorted(s for s in want if ".b." in s)
    assert os.path.exists(pre + ".files") and os.path.exists(pre + ".log")


@pytest.mark.parametrize("name", MB_CASES)
def test_gpu_built_blocks_vote_golden(name, hbm_builds):
    c = Case(name)
    assert is_multi_block_key(c.index_key)
    ix = hbm_builds(c.index_key)
    assert ix.n_blocks == fixture_blocks(c.index_key)
    out, jout, bm = ix.vote(c.params, c.r1, c.r2)
    got = pack_records(out, jout, bm)
    assert (got == c.expected).all(), describe_mismatch(got, c.expected, c.ends, c.params.multi_best)


def test_gpu_built_blocks_vote_like_opened(saved_builds, index_cache):
    import subread_amd as sa
    from subread_amd.abi import default_params, PROGRAM_ALIGN
    from subread_amd.sim import Genome, simulate_reads
    built, pre = saved_builds("long777_fullM17")
    g = Genome.read_fasta(index_cache.genome_fasta("long777"))
    reads = simulate_reads(g, 20000, 100, seed=1717)
    p = default_params(PROGRAM_ALIGN, False)
    opened = sa.VoteIndex(pre, device=0)
    try:
        assert opened.n_blocks == built.n_blocks == 6
        a, _, _ = built.vote(p, reads, None)
        b, _, _ = opened.vote(p, reads, None)
        got, want = pack_records(a, None, None), pack_records(b, None, None)
        assert (want.view(np.uint8) != 0).any()
        assert (got == want).all(), describe_mismatch(got, want, 1, p.multi_best)
    finally:
        opened.close()


def test_gpu_one_block_plan_equals_cpu_builder(tmp_path):
    """more items than the budget but no split point (one contig under 2 Mbp): one block, the CPU
    builder's bytes"""
    import subread_amd as sa
    from subread_amd.sim import random_genome
    g = random_genome([500000], 9191)
    fa = str(tmp_path / "one.fa")
    g.write_fasta(fa)
    cpu, gpu = str(tmp_path / "cpu"), str(tmp_path / "gpu")
    sa.build_index(fa, cpu, gap=1, memory_mb=1, force_one_block=False)
    ix = sa.VoteIndex.build_genome(g, gap=1, memory_mb=1, force_one_block=False, device=0, save_prefix=gpu)
    try:
        assert ix.n_blocks == 1
        assert ix.info.items > 131072   # the -M 1 budget
        assert block_files(gpu) == block_files(cpu) == [".00.b.array", ".00.b.tab"]
        for suf in (".00.b.tab", ".00.b.array", ".reads"):
            with open(cpu + suf, "rb") as f1, open(gpu + suf, "rb") as f2:
                assert f1.read() == f2.read(), suf
    finally:
        ix.close()


def test_gpu_build_failure_and_close_leave_the_builder_usable(index_cache):
    import subread_amd as sa
    gname, gap, memory_mb, force = index_recipe("synth4242_gappedM1")
    fa = index_cache.genome_fasta(gname)
    with pytest.raises(sa.SvgError):
        sa.VoteIndex.build(fa, gap=gap, memory_mb=memory_mb, force_one_block=force, device=99)
    c = Case("pe_mb_synth_gappedM1")
    for _ in range(2):
        ix = sa.VoteIndex.build(fa, gap=gap, memory_mb=memory_mb, force_one_block=force, device=0)
        assert ix.n_blocks == 2
        out, _, _ = ix.vote(c.params, c.r1, c.r2)
        assert (pack_records(out, None, None) == c.expected).all()
        ix.close()
        assert ix.h is None
