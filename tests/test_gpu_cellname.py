"""svg_cell_set_samples, svg_cell_parse_names, svg_cell_count_names_batch and svg_cell_counter_tallies
on the GPU: the parse against the reference's own answers (tests/golden/cellname/cellname.npz) and
against the plain-C model (tests/native/cellname_model.c, held to the reference on the CPU by
tests/test_cellname_golden.py) on names the reference cannot take; the fused entry against
count_batch fed with the model's barcodes, UMIs and sample numbers; the tallies against the model;
the refusals and the argument errors."""
import numpy as np
import pytest

import subread_amd as sa
from subread_amd import abi
from subread_amd.abi import CELL_FEATURE_DTYPE, ReadBatch
from tests.cellassign_common import fixture_allow, fixture_case as assign_case, make_features, make_whitelist, raw
from tests.cellname_common import (BCL, FASTQ, LINES, MODES, N_SAMPLES, QUALS, ROWS, compose, fixture_names, join_names, load_fixture,
                                   model_parse, model_tallies)
from tests.cellumi_common import same_result
from tests.common import ensure_built

ensure_built()
pytestmark = pytest.mark.gpu

KEY = "synth4242_full"
LETTERS = np.frombuffer(b"ACGTN", np.uint8)
UNPACK = np.frombuffer(b"AGCT", np.uint8)            # base2int


@pytest.fixture(scope="module")
def ix(index_cache):
    x = sa.VoteIndex(index_cache.get(KEY), device=0)
    x.set_cell_samples(ROWS, LINES, N_SAMPLES)
    yield x
    x.close()


def batch(names):
    return ReadBatch(*join_names(names))


def packed_words(got):
    """the six words a name of the model's layout: barcode words, its exception word, the UMI's"""
    n = len(got["fields"])
    b, u = got["barcodes"], got["umis"]
    assert b.stride == u.stride == abi.CELL_NAME_STRIDE and b.starts is None
    return np.stack([b.bases[0:2 * n:2], b.bases[1:2 * n:2], b.xmask[:n], u.bases[0:2 * n:2], u.bases[1:2 * n:2], u.xmask[:n]], 1)


def text_of(words, xword, L):
    k = np.arange(L)
    t = UNPACK[(words[:, None] >> (30 - 2 * k)) & 3]
    return np.where((xword[:, None] >> (31 - k)) & 1, ord("N"), t).astype(np.uint8)


def same_as_model(got, want):
    for k in ("fields", "trimmed_len", "lane", "sample_no", "status"):
        assert (got[k] == want[k]).all(), k
    assert (packed_words(got) == want["packed"]).all()
    assert got["refused"] == int((want["status"] != 0).sum())


@pytest.mark.parametrize("which", list(MODES))
def test_gpu_parse_equals_the_reference(which, ix):
    mode, bl, ul = MODES[which]
    z, names = load_fixture(), fixture_names(which)
    ref = z[which + "_ref"]
    assert len(names) >= 1025
    for n in (1, 63, 64, 65, 1025, len(names)):
        lo = 0 if n == len(names) else (len(names) - n) // 2
        got = ix.cell_parse_names(batch(names[lo:lo + n]), mode, bl, ul)
        assert got["refused"] == 0 and (got["status"] == 0).all()
        for col, k in enumerate(("fields", "trimmed_len", "lane", "sample_no")):
            assert (got[k] == ref[lo:lo + n, col]).all(), (n, k)
        w = packed_words(got)
        assert (text_of(w[:, 0], w[:, 2], bl) == z[which + "_bc"][lo:lo + n]).all()
        assert (text_of(w[:, 3], w[:, 5], ul) == z[which + "_umi"][lo:lo + n]).all()
        assert (w[:, 1] == 0).all() and (w[:, 4] == 0).all()
        assert (got["barcodes"].lens == bl).all() and (got["umis"].lens == ul).all()
    empty = ix.cell_parse_names(batch([]), mode, bl, ul)
    assert len(empty["fields"]) == 0 and empty["refused"] == 0


def long_names(n, mode, rng, pad):
    """names with text behind the lane field (the scan has stopped there): pad(i) more bytes"""
    bl, ul = 16, 12
    out = []
    for i in range(n):
        r = ROWS[i % len(ROWS)]
        bcumi = LETTERS[rng.integers(0, 5, bl + ul)].tobytes()
        q = QUALS[rng.integers(0, len(QUALS), bl + ul)].tobytes()
        out.append(compose(i, bcumi, q, r[2], b"F" * len(r[2]), b"|@RgLater@L%03d " % (1 + i % 4) + b"x" * pad(i), mode))
    return out


def test_gpu_parse_spans(ix):
    """a block stages 16 KiB of text from its first name on: names of unequal length so that some lie
    across the end of that span and some beyond it; a batch whose every block's names take more than
    the span; names longer than the span; and names whose offsets run backwards"""
    rng = np.random.default_rng(2229)
    for mode in (BCL, FASTQ):
        mixed = long_names(333, mode, rng, lambda i: int(rng.integers(0, 900)) if i % 3 else 0)
        spans = np.add.reduceat([len(x) for x in mixed], np.arange(0, len(mixed), 64))
        assert (spans > 16384).sum() >= 3 and max(len(x) for x in mixed) < 1200
        big = long_names(130, mode, rng, lambda i: 400 + i % 7)
        assert min(np.add.reduceat([len(x) for x in big], np.arange(0, 128, 64))) > 16384
        huge = long_names(5, mode, rng, lambda i: 17000 + 1000 * i)
        for names in (mixed, big, huge):
            same_as_model(ix.cell_parse_names(batch(names), mode, 16, 12), model_parse(names, mode, 16, 12))
        text, offs, lens = join_names(mixed)
        order = rng.permutation(len(mixed))
        got = ix.cell_parse_names(ReadBatch(text, offs[order], lens[order]), mode, 16, 12)
        same_as_model(got, model_parse(None, mode, 16, 12, joined=(text, offs[order], lens[order])))


def refused_names(mode):
    ok = compose(7, b"ACGTACGTACGTACGT" + b"AACCGGTTAACC", b"F" * 28, b"ACGTACGT", b"F" * 8, b"|@RgLater@L001", mode)
    two = ok[:13] + b"ACGTACGTACGTACGTAACCGGTTAACC|FFFF"                       # two fields
    bang = ok[:13 + 20] + b"!" + ok[13 + 21:]                                   # a '!' in the UMI
    lower = ok[:13 + 3] + b"a" + ok[13 + 4:]                                    # a character outside A/C/G/T/N in the barcode
    short = ok[:13] + b"ACGTACGTAC||"                                           # three fields, the UMI past the end
    return ok, [two, bang, lower, short, b"R", b"", b"R0|"]


def test_gpu_parse_refusals_and_arguments(ix):
    for mode in (BCL, FASTQ):
        ok, bad = refused_names(mode)
        names = [ok] + bad + [ok]
        got = ix.cell_parse_names(batch(names), mode, 16, 12)
        want = model_parse(names, mode, 16, 12)
        same_as_model(got, want)
        assert got["status"].tolist() == [0, 1, 3, 3, 2, 1, 1, 1, 0] and got["refused"] == 7
        assert (got["sample_no"][1:-1] == -1).all() and got["sample_no"][0] == 1
    ok = refused_names(BCL)[0]
    for args in ((BCL, 16, 0), (BCL, 16, 15), (BCL, 0, 12), (BCL, 17, 12), (2, 16, 12)):
        with pytest.raises(sa.SvgError) as err:
            ix.cell_parse_names(batch([ok]), *args)
        assert err.value.rc == -1


def test_gpu_set_samples_arguments(index_cache):
    x = sa.VoteIndex(index_cache.get(KEY), device=0)
    try:
        ok = compose(1, b"A" * 28, b"F" * 28, b"ACGTACGT", b"F" * 8, b"|@RgLater@L001", BCL)
        x.set_cell_samples([(abi.CELL_LANE_ALL, 2, "ACGTACGT")], [0, 2], 2)
        assert x.cell_parse_names(batch([ok]), BCL, 16, 12)["sample_no"].tolist() == [2]
        for rows, lines, S in (([(1, 0, "ACGT")], [], 2), ([(1, 3, "ACGT")], [], 2), ([(1, 1, "ACGU")], [], 2), ([(1, 1, "acgt")], [], 2),
                               ([(1, 1, "ACGN")], [], 2), ([(1, 1, "A" * 33)], [], 2), ([(1, 1, "")], [], 2), ([(1, 1, "ACGT")], [], 256),
                               ([(1, 1, "ACGT")], [], 0), ([], [3], 2), ([], [-1], 2), ([(-1, 1, "ACGT")], [], 2)):
            with pytest.raises(sa.SvgError) as err:
                x.set_cell_samples(rows, lines, S)
            assert err.value.rc == -1 and "svg_cell_set_samples" in str(err.value)
        assert x.cell_parse_names(batch([ok]), BCL, 16, 12)["sample_no"].tolist() == [2]      # a refused call changed nothing
        x.set_cell_samples([(abi.CELL_LANE_ALL, 1, "A" * 32)], [], 1)                           # the longest index; replaces everything
        assert x.cell_parse_names(batch([ok]), BCL, 16, 12)["sample_no"].tolist() == [-1]
        x.set_cell_samples([], [], 0)                                                           # cleared
        assert x.cell_parse_names(batch([ok]), BCL, 16, 12)["sample_no"].tolist() == [-1]
    finally:
        x.close()


def names_for(barcodes, umis, rng, mode, bad_every=0):
    """BCL- or FASTQ-style names around given barcodes and UMIs, over the sheet of ROWS: exact and near
    indexes, indexes on no row, and (FASTQ) "input#" names with present and absent lines"""
    out = []
    for i, (b, u) in enumerate(zip(barcodes, umis)):
        bcumi = bytes(b) + bytes(u)
        q = QUALS[rng.integers(0, len(QUALS), len(bcumi))].tobytes()
        r = ROWS[int(rng.integers(0, len(ROWS)))]
        idx = bytearray(r[2])
        for _ in range(int(rng.integers(0, 3))):
            idx[int(rng.integers(0, len(idx)))] = b"ACGT"[int(rng.integers(0, 4))]
        if mode == FASTQ and i % 3 == 0:
            out.append(b"R%011d|" % i + bcumi + b"|" + q + b"|input#%04d@L001" % int(rng.integers(0, 14)))
        else:
            out.append(compose(i, bcumi, q, bytes(idx), b"F" * len(idx), b"|@RgLater@L%03d" % int(rng.integers(1, 5)), mode))
    return out


def host_prepared(names, mode, bl, ul):
    m = model_parse(names, mode, bl, ul)
    assert (m["status"] == 0).all()
    return m, sa.pack_reads(ReadBatch.fixed(m["bc"])), sa.pack_reads(ReadBatch.fixed(m["umi"]))


@pytest.mark.parametrize("which,mode", [("default", BCL), ("second", FASTQ)])
def test_gpu_count_names_on_the_cellassign_fixture(which, mode, ix):
    """the fused entry against count_batch fed with the model's barcodes, UMIs and samples: the same
    tables and entries, the same result, the same tallies, which equal the model's"""
    from tests.cellalign_common import case_params
    fc = assign_case(KEY, 10, which)
    n, L, S = len(fc["heads"]), 12, N_SAMPLES
    rng = np.random.default_rng(1955 + mode)
    umis = LETTERS[np.where(rng.random((n, L)) < 0.02, 4, rng.integers(0, 3, (n, L)))]
    names = names_for(fc["barcodes"], umis, rng, mode)
    m, bpk, upk = host_prepared(names, mode, 16, L)
    assert (m["sample_no"] > 0).sum() >= 100 and (m["sample_no"] <= 0).sum() >= 50
    p = case_params(10, which)
    ix.set_cell_annotation(fc["features"], allow_multi_overlap=fixture_allow(10, which))
    ix.set_cell_barcodes(fc["whitelist"])
    a, b, c = (ix.cell_counter(L, S) for _ in range(3))
    try:
        plain = ix.cell_assign(fc["pk"], bpk, **p)
        heads, hits = plain[0], plain[2]
        res = a.count_names_batch(fc["pk"], batch(names), mode, want_result=True, **p)
        assert all(raw(x).tobytes() == raw(y).tobytes() for x, y in zip(res, plain))
        assert b.count_names_batch(fc["pk"], batch(names), mode, **p) is None
        c.count_batch(fc["pk"], bpk, upk, m["sample_no"], **p)
        want = c.finish(want_entries=True)
        assert len(want["counts"]) >= 20
        for k in (a, b):
            same_result(k.finish(want_entries=True), want)
        # the tallies: the model's, from the records of cell_assign
        tal = model_tallies(heads, hits, m["sample_no"], None, S)
        multi, unmapped, nosample = int((heads["n_records"] > 1).sum()), int((heads["n_records"] == 0).sum()), int((m["sample_no"] <= 0).sum())
        print("multi-record reads", multi, "unmapped reads", unmapped, "reads without a sample", nosample,
              "contig -1 records", int((hits["contig"] < 0).sum()))
        assert unmapped >= 100 and nosample >= 50 and (multi >= 100 if which == "second" else multi == 0)
        # (no read of the fixture aligns into a contig's padding: records with contig -1 are in
        # test_gpu_tallies_with_records_in_the_padding)
        assert tal[0].sum() == np.maximum(heads["n_records"], 1).sum() and tal[1].sum() > tal[2].sum() > 0
        for k in (a, b, c):
            t = k.tallies()
            assert (t["reads"] == tal[0]).all() and (t["mapped"] == tal[1]).all() and (t["assigned"] == tal[2]).all()
        a.reset()
        assert all((v == 0).all() for v in a.tallies().values())
        # refused names: counted on the device, finish fails until reset, and nothing of them is tallied
        ok, bad = refused_names(mode)
        spoiled = list(names)
        spoiled[5], spoiled[77] = bad[0], bad[1]
        a.count_names_batch(fc["pk"], batch(spoiled), mode, **p)
        for _ in range(2):
            with pytest.raises(sa.SvgError) as err:
                a.finish()
            assert err.value.rc == -1 and "2 read names refused" in str(err.value)
        st = np.zeros(n, np.uint32)
        st[[5, 77]] = 1
        assert (a.tallies()["reads"] == model_tallies(heads, hits, m["sample_no"], st, S)[0]).all()
        a.reset()
        # a failed call leaves the counter as it was
        a.count_names_batch(fc["pk"], batch(names), mode, **p)
        before = a.tallies()
        with pytest.raises(sa.SvgError):
            a.count_names_batch(fc["pk"], batch(names[:-1]), mode, **p)
        with pytest.raises(sa.SvgError):
            a.count_names_batch(fc["pk"], batch(names), 7, **p)
        assert all((a.tallies()[k] == before[k]).all() for k in before)
        same_result(a.finish(want_entries=True), want)
        small = ix.cell_counter(L, 2)                                  # a counter of fewer samples than the sheet
        with pytest.raises(sa.SvgError):
            small.count_names_batch(fc["pk"], batch(names), mode, **p)
        small.close()
        ix.set_cell_barcodes([])                                       # no whitelist: the barcode length is unknown
        with pytest.raises(sa.SvgError):
            a.count_names_batch(fc["pk"], batch(names), mode, **p)
    finally:
        ix.set_cell_annotation(np.zeros(0, CELL_FEATURE_DTYPE))
        ix.set_cell_barcodes([])
        for k in (a, b, c):
            k.close()


def test_gpu_tallies_with_records_in_the_padding():
    """records with contig -1: a read of a few foreign bases and then a contig's first bases is reported
    at the position of its first base, in the padding in front of the contig, which
    locate_gene_position does not place (the unmapped call of :2067 / :2087).  Such a first record
    alone, and followed by a placed record (the same bases, two of them changed, inside another
    contig), among ordinary reads, with and without a sample: the tallies equal the model's"""
    from subread_amd.sim import Genome, simulate_reads
    from tests.cellalign_common import case_params
    rng = np.random.default_rng(2067)
    acgt = LETTERS[:4]
    seqs = [acgt[rng.integers(0, 4, 20000)].copy() for _ in range(3)]
    twin = seqs[1][:100].copy()
    twin[[40, 60]] = acgt[(np.searchsorted(acgt, twin[[40, 60]]) + 1) % 4]
    seqs[0][5000:5100] = twin
    g = Genome(["chrA", "chrB", "chrC"], seqs)
    x = sa.VoteIndex.build_genome(g, gap=1, memory_mb=8000, force_one_block=True, device=0)
    L, S = 12, N_SAMPLES
    try:
        crafted = []
        for i in range(40):
            crafted.append(np.concatenate([acgt[rng.integers(0, 4, 3)], seqs[1][:97]]).tobytes())            # chrB's padding, then chrA
            J = 3 + i % 28
            crafted.append(np.concatenate([acgt[rng.integers(0, 4, J)], seqs[2 * (i % 2)][:100 - J]]).tobytes())   # the padding alone
        plain = simulate_reads(g, 400, 100, seed=2087, threads=4)
        reads = crafted + [plain.read(i) for i in range(len(plain))]
        n = len(reads)
        pk = sa.pack_reads(ReadBatch.from_list(reads))
        e = x.export()
        feats = make_features(e["chr_end"][:e["n_chr"]].copy(), int(e["padding"]), rng, per_kb=4.0, genes_per=3)
        wl = make_whitelist(50, 16, rng)
        bc = np.array([np.frombuffer(w, np.uint8) for w in wl])[rng.integers(0, 50, n)]
        umis = LETTERS[rng.integers(0, 4, (n, L))]
        names = names_for(bc, umis, rng, BCL)
        m, bpk, upk = host_prepared(names, BCL, 16, L)
        x.set_cell_samples(ROWS, LINES, S)
        x.set_cell_annotation(feats, allow_multi_overlap=1)
        x.set_cell_barcodes(wl)
        p = case_params(10, "second")
        heads, _, hits, _, _ = x.cell_assign(pk, bpk, **p)
        nrec, sm = heads["n_records"], m["sample_no"]
        first = hits["contig"][np.minimum(heads["first_record"].astype(np.int64), len(hits) - 1)]
        lost = (nrec > 0) & (first < 0)
        alone, followed = lost & (nrec == 1), lost & (nrec > 1)
        later_placed = np.array([(hits["contig"][int(f) + 1:int(f) + int(k)] >= 0).any() for f, k in zip(heads["first_record"], nrec)])
        print("contig -1 records", int((hits["contig"] < 0).sum()), "first alone", int(alone.sum()), "first and then placed records",
              int((followed & later_placed).sum()), "of them with a sample", int((lost & (sm > 0)).sum()))
        assert (hits["contig"] < 0).sum() >= 50 and alone.sum() >= 30 and (followed & later_placed).sum() >= 20
        assert (alone & (sm > 0)).sum() >= 5 and (followed & later_placed & (sm > 0)).sum() >= 5 and (lost & (sm <= 0)).sum() >= 5
        assert ((nrec > 0) & (first >= 0) & (sm > 0)).sum() >= 100
        tal = model_tallies(heads, hits, sm, None, S)
        # the rule is visible in the numbers: fewer mapped reads than reads with records and a sample
        assert tal[1].sum() == ((nrec > 0) & (first >= 0) & (sm > 0)).sum() == ((nrec > 0) & (sm > 0)).sum() - (lost & (sm > 0)).sum()
        assert tal[2].sum() > 0
        a, b = x.cell_counter(L, S), x.cell_counter(L, S)
        a.count_names_batch(pk, batch(names), BCL, **p)
        b.count_batch(pk, bpk, upk, sm, **p)
        for k in (a, b):
            t = k.tallies()
            assert (t["reads"] == tal[0]).all() and (t["mapped"] == tal[1]).all() and (t["assigned"] == tal[2]).all()
        same_result(a.finish(want_entries=True), b.finish(want_entries=True))
    finally:
        x.close()


def test_gpu_count_names_cut_in_two(ix, index_cache):
    """131,073 reads (one more than a chunk) in one call and as two calls, and through count_batch;
    then a call that fails in its second chunk, after the first chunk's kernels have added to the
    counter on the device: the counter is as it was"""
    from subread_amd.sim import Genome, simulate_reads
    n, more, L, S = 131073, 131072 + 256, 12, N_SAMPLES
    g = Genome.read_fasta(index_cache.genome_fasta("synth4242"))
    every = simulate_reads(g, more, 100, seed=1955, indel=0.02, nrate=0.001, threads=8)
    rb = every.slice(0, n)
    rng = np.random.default_rng(1955)
    e = ix.export()
    feats = make_features(e["chr_end"][:e["n_chr"]].copy(), int(e["padding"]), rng, per_kb=4.0, genes_per=3)
    wl = make_whitelist(200, 16, rng)
    bc = np.array([np.frombuffer(w, np.uint8) for w in wl])[rng.integers(0, 8, n)]
    umis = LETTERS[rng.integers(0, 2, (n, L))]
    idx = [ROWS[0][2], ROWS[3][2], ROWS[4][2], b"CCCCCCCC"]
    pick = rng.integers(0, 4, n)
    names = [compose(i, bc[i].tobytes() + umis[i].tobytes(), b"F" * 28, idx[pick[i]], b"F" * len(idx[pick[i]]), b"|@RgLater@L001", BCL)
             for i in range(n)]
    m, bpk, upk = host_prepared(names, BCL, 16, L)
    ix.set_cell_annotation(feats, allow_multi_overlap=1)
    ix.set_cell_barcodes(wl)
    a, b, c = (ix.cell_counter(L, S) for _ in range(3))
    try:
        pk = sa.pack_reads(rb)
        ix.set_timing(True)
        a.count_names_batch(pk, batch(names), BCL)
        assert ix.cell_names_timing() > 0 and ix.cell_names_timing() == 0
        ix.set_timing(False)
        one = a.finish(want_entries=True)
        c.count_batch(pk, bpk, upk, m["sample_no"])
        same_result(c.finish(want_entries=True), one)
        h = 65536
        for lo, hi in ((0, h), (h, n)):
            b.count_names_batch(sa.pack_reads(rb.slice(lo, hi)), batch(names[lo:hi]), BCL)
        same_result(b.finish(want_entries=True), one)
        assert len(one["counts"]) >= 1000 and (one["entries"]["outcome"] == 1).sum() >= 100
        ta, tb, tc = a.tallies(), b.tallies(), c.tallies()
        assert all((ta[k] == tb[k]).all() and (ta[k] == tc[k]).all() for k in ta)
        assert ta["reads"][S] > 10000 and ta["reads"][0] > 10000 and ta["reads"].sum() >= n and ta["assigned"].sum() > 1000
        # 17 genes on either strand over one read's place: svg_cell_assign refuses such an alignment (SVG_E_DEVICE).  The
        # reads that lie there go to the end of a batch of one chunk and 256 reads, so the first chunk is counted on the
        # device before the second fails
        bc2 = np.array([np.frombuffer(w, np.uint8) for w in wl])[rng.integers(0, 8, more)]
        um2 = LETTERS[rng.integers(0, 2, (more, L))]
        names2 = np.array([compose(i, bc2[i].tobytes() + um2[i].tobytes(), b"F" * 28, idx[i % 4], b"F" * len(idx[i % 4]), b"|@RgLater@L001", BCL)
                           for i in range(more)], dtype=object)
        heads, _, hits, _, _ = ix.cell_assign(sa.pack_reads(every))
        read_of = np.repeat(np.arange(more), heads["n_records"])
        k0 = int(np.flatnonzero(hits["contig"] >= 0)[more // 2])
        c0, p0 = int(hits["contig"][k0]), int(hits["chro_pos"][k0])
        near = np.unique(read_of[(hits["contig"] == c0) & (np.abs(hits["chro_pos"].astype(np.int64) - p0) < 250)])
        assert 1 <= len(near) <= 256
        order = np.concatenate([np.setdiff1d(np.arange(more), near), near])
        crowd = np.zeros(34, CELL_FEATURE_DTYPE)
        crowd["contig"], crowd["start"], crowd["end"] = c0, max(1, p0 - 20), p0 + 150
        crowd["gene"], crowd["is_negative_strand"] = 1000000 + np.arange(34) // 2, np.arange(34) % 2
        ix.set_cell_annotation(np.concatenate([feats, crowd]), allow_multi_overlap=1)
        a.reset()
        few = order[:3000]
        a.count_names_batch(sa.pack_reads(ReadBatch(every.seq, every.offsets[few], every.lens[few])), batch(list(names2[few])), BCL)
        before, table = a.tallies(), a.finish(want_entries=True)
        assert before["reads"].sum() >= 3000 and len(table["counts"]) >= 20
        with pytest.raises(sa.SvgError) as err:
            a.count_names_batch(sa.pack_reads(ReadBatch(every.seq, every.offsets[order], every.lens[order])), batch(list(names2[order])), BCL)
        assert "SVG_CELL_MAX_GENES" in str(err.value)
        after = a.tallies()
        assert all((after[k] == before[k]).all() for k in before)
        same_result(a.finish(want_entries=True), table)
        a.count_names_batch(sa.pack_reads(ReadBatch(every.seq, every.offsets[few], every.lens[few])), batch(list(names2[few])), BCL)
        assert all((a.tallies()[k] == 2 * before[k]).all() for k in before)          # and it goes on counting from there
    finally:
        ix.set_timing(False)
        ix.set_cell_annotation(np.zeros(0, CELL_FEATURE_DTYPE))
        ix.set_cell_barcodes([])
        for k in (a, b, c):
            k.close()
