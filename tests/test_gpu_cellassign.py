"""svg_cell_assign_batch / svg_cell_assign_records (cellCounts' gene assignment and cell-barcode
lookup on the GPU) through VoteIndex: equal to the plain-C model (tests/native/cellassign_model.c
over the host builder's tables) on simulated reads and on crafted records, its alignment part equal
to cell_align's byte for byte, the same answers however the batch is cut, and the refusals.  The
model equals the reference's own records on the CPU (tests/test_cellassign_golden.py), and the GPU
equals those records here on every fixture case."""
import numpy as np
import pytest

from subread_amd.abi import CELL_ALN_DTYPE, CELL_FEATURE_DTYPE
from tests.cellassign_common import (FIXTURE_CASES, fixture_allow, fixture_case, make_features, make_read_barcodes, make_whitelist, model_assign, model_barcodes, pack_barcodes,
                                     raw)
from tests.common import ensure_built

ensure_built()
pytestmark = pytest.mark.gpu

CHUNK = 1 << 17
KEYS = ["synth4242_full", "synth4242_gapped"]   # (open_index also serves the fixture's chr901_gapped)


@pytest.fixture(scope="module")
def open_index(index_cache):
    import subread_amd as sa
    held = {}

    def get(key):
        if key not in held:
            ix = sa.VoteIndex(index_cache.get(key), device=0)
            e = ix.export()
            held[key] = (ix, e["chr_end"][:e["n_chr"]].copy(), int(e["padding"]))
        return held[key]

    yield get
    for ix, _, _ in held.values():
        ix.close()


@pytest.fixture(scope="module")
def sim(index_cache):
    """20k simulated 100-base reads of synth4242, a whitelist of 3,000 16-base barcodes with
    neighbours at distance 1 and 2, and a read barcode of every class per read"""
    import subread_amd as sa
    from subread_amd.sim import Genome, simulate_reads
    g = Genome.read_fasta(index_cache.genome_fasta("synth4242"))
    rb = simulate_reads(g, 20000, 100, seed=2061, indel=0.05, nrate=0.002, threads=8)
    rng = np.random.default_rng(1701)
    wl = make_whitelist(3000, 16, rng)
    bc = make_read_barcodes(wl, 20000, rng)
    return dict(rb=rb, pk=sa.pack_reads(rb), wl=wl, bc=bc, bpk=pack_barcodes(bc), want_bc=model_barcodes(wl, bc))


@pytest.mark.parametrize("key,total,which", FIXTURE_CASES, ids=["%s-n%d-%s" % c for c in FIXTURE_CASES])
def test_gpu_cell_assign_matches_reference(key, total, which, open_index):
    """every byte of the reference's own records (tests/golden/cellassign/cellassign.npz): the alignment
    records under the reference's own fill of the exon planes, the hit records, the gene lists and the
    barcode numbers; and the alignment part is cell_align's"""
    from tests.cellalign_common import case_params
    c = fixture_case(key, total, which)
    ix, chr_end, pad = open_index(key)
    assert (chr_end == c["chr_end"]).all()
    ix.set_cell_annotation(c["features"], allow_multi_overlap=fixture_allow(total, which))
    ix.set_cell_barcodes(c["whitelist"])
    try:
        heads, alns, hits, genes, bcno = ix.cell_assign(c["pk"], pack_barcodes(c["barcodes"]), **case_params(total, which))
        plain = ix.cell_align(c["pk"], **case_params(total, which))
    finally:
        ix.set_cell_annotation(np.zeros(0, CELL_FEATURE_DTYPE))
        ix.set_cell_barcodes([])
    assert (raw(heads) == raw(c["heads"])).all() and len(alns) == len(c["alns"]) and (raw(alns) == raw(c["alns"])).all()
    assert (raw(plain[0]) == raw(heads)).all() and (raw(plain[1]) == raw(alns)).all()
    assert same_hits(hits, genes, c["hits"], c["genes"])
    assert (bcno == c["bcno"]).all()


def same_hits(got_h, got_g, want_h, want_g):
    return len(got_h) == len(want_h) and (raw(got_h) == raw(want_h)).all() and len(got_g) == len(want_g) and (got_g == want_g).all()


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("allow,max_rep", [(0, 1), (1, 4)])
def test_gpu_cell_assign_matches_model_at_volume(key, allow, max_rep, open_index, sim):
    ix, chr_end, pad = open_index(key)
    feats = make_features(chr_end, pad, np.random.default_rng(7 + allow), per_kb=4.0, genes_per=3)
    p = dict(max_reported_alignments_per_read=max_rep)
    plain = ix.cell_align(sim["pk"], **p)          # before any annotation: no exons
    ix.set_cell_annotation(feats, allow_multi_overlap=allow)
    ix.set_cell_barcodes(sim["wl"])
    try:
        heads, alns, hits, genes, bcno = ix.cell_assign(sim["pk"], sim["bpk"], **p)
        ix.set_cell_exons([], [])                  # the annotation filled the planes: the scores moved with them
        heads0, alns0, hits0, genes0, _ = ix.cell_assign(sim["pk"], None, **p)
    finally:
        ix.set_cell_annotation(np.zeros(0, CELL_FEATURE_DTYPE))
        ix.set_cell_barcodes([])
    assert (raw(heads0) == raw(plain[0])).all() and len(alns0) == len(plain[1]) and (raw(alns0) == raw(plain[1])).all()
    for h, a, hh, gg in ((heads, alns, hits, genes), (heads0, alns0, hits0, genes0)):
        wh, wg = model_assign(feats, allow, chr_end, pad, a)
        assert same_hits(hh, gg, wh, wg)
    assert (bcno == sim["want_bc"]).all()
    assert (hits["nhits"] == 0).sum() >= 20 and (hits["nhits"] == 1).sum() >= 20 and (hits["contig"] >= 0).all()
    if allow:
        assert (hits["nhits"] >= 2).sum() >= 20
        adv = model_assign(feats, allow, chr_end, pad, alns, advance=True)
        differ = sum(1 for i in range(len(hits)) if hits["nhits"][i] != adv[0]["nhits"][i] or
                     (genes[int(hits["first_gene"][i]):][:int(hits["nhits"][i])] != adv[1][int(adv[0]["first_gene"][i]):][:int(hits["nhits"][i])]).any())
        # records where an advancing cursor would give another list: an alignment with an indel whose second M
        # reaches a feature the first does not.  The bar of 20 holds on the full index; a gapped index at 10
        # subreads aligns too few reads with an indel (test_cellalign_golden.py lowers its indel bars there too)
        assert differ >= (20 if "full" in key else 1)
    else:
        assert (hits["nhits"] <= 1).all()
    for cls in range(6):           # exact, even, odd, two substitutions, N even, N odd
        got = bcno[cls::6]
        assert ((got < 0) if cls == 3 else (got >= 0)).sum() >= 20, cls


def test_gpu_cell_assign_no_annotation_no_barcodes(open_index, sim):
    import subread_amd as sa
    ix, chr_end, pad = open_index(KEYS[0])
    pk = sa.pack_reads(sim["rb"].slice(0, 3000))
    plain = ix.cell_align(pk)
    for bpk in (None, pack_barcodes(sim["bc"][:3000])):      # barcodes given but no whitelist set: -1 as well
        heads, alns, hits, genes, bcno = ix.cell_assign(pk, bpk)
        assert (raw(heads) == raw(plain[0])).all() and (raw(alns) == raw(plain[1])).all()
        wh, wg = model_assign(np.zeros(0, CELL_FEATURE_DTYPE), 0, chr_end, pad, alns)
        assert same_hits(hits, genes, wh, wg) and len(genes) == 0 and (hits["contig"] >= 0).any()
        assert (bcno == -1).all() and len(bcno) == len(heads) == 3000


def test_gpu_cell_assign_empty_batch(open_index):
    import subread_amd as sa
    from subread_amd.abi import ReadBatch
    ix, _, _ = open_index(KEYS[0])
    out = ix.cell_assign(sa.pack_reads(ReadBatch.from_list([])))
    assert [len(x) for x in out] == [0, 0, 0, 0, 0]
    h, g = ix.cell_assign_records(np.zeros(0, CELL_ALN_DTYPE))
    assert len(h) == 0 and len(g) == 0


def test_gpu_cell_assign_split_and_one_past_a_chunk(open_index, index_cache):
    """131,073 reads (one past a chunk): the whole equals its two halves put together"""
    import subread_amd as sa
    from subread_amd.abi import ReadBatch
    from subread_amd.sim import Genome, simulate_reads
    ix, chr_end, pad = open_index(KEYS[0])
    g = Genome.read_fasta(index_cache.genome_fasta("synth4242"))
    rb = simulate_reads(g, CHUNK + 1, 100, seed=99, indel=0.02, nrate=0.001, threads=8)
    rng = np.random.default_rng(3)
    wl = make_whitelist(2000, 16, rng)
    base = make_read_barcodes(wl, 6000, rng)
    bc = [base[i % 6000] for i in range(CHUNK + 1)]
    feats = make_features(chr_end, pad, rng, per_kb=4.0, genes_per=3)
    ix.set_cell_annotation(feats, allow_multi_overlap=True)
    ix.set_cell_barcodes(wl)
    try:
        whole = ix.cell_assign(sa.pack_reads(rb), pack_barcodes(bc), max_reported_alignments_per_read=2)
        half = (CHUNK + 1) // 2
        parts = [ix.cell_assign(sa.pack_reads(rb.slice(a, b)), pack_barcodes(bc[a:b]), max_reported_alignments_per_read=2)
                 for a, b in ((0, half), (half, CHUNK + 1))]
    finally:
        ix.set_cell_annotation(np.zeros(0, CELL_FEATURE_DTYPE))
        ix.set_cell_barcodes([])
    heads, alns, hits, genes, bcno = whole
    assert len(heads) == CHUNK + 1 and (bcno == np.tile(model_barcodes(wl, base), 22)[:CHUNK + 1]).all()
    assert (raw(alns) == raw(np.concatenate([p[1] for p in parts]))).all()
    assert (genes == np.concatenate([p[3] for p in parts])).all()
    assert (bcno == np.concatenate([p[4] for p in parts])).all()
    h2 = parts[1][2].copy()
    h2["first_gene"][h2["nhits"] > 0] += len(parts[0][3])
    assert (raw(hits) == raw(np.concatenate([parts[0][2], h2]))).all()
    wh, wg = model_assign(feats, 1, chr_end, pad, alns)
    assert same_hits(hits, genes, wh, wg) and (hits["nhits"] >= 2).any()
    assert hits["nhits"][len(parts[0][2]):].sum() > 0     # the read past the chunk border and its chunk are assigned


def crafted(chr_end, pad):
    e0, last = int(chr_end[0]), int(chr_end[-1])
    pos = [pad - 2, pad - 1, e0 + 15 - pad - 1, e0 + 15 - pad, last + 100, pad + 999, pad + 999, pad + 999, pad + 999, pad + 999]
    cig = [b"50M", b"50M", b"50M", b"50M", b"50M", b"20M300N10M2D20M", b"30M8S12M", b"9S41M", b"100000000M", b"50M"]
    a = np.zeros(len(pos) + 3, CELL_ALN_DTYPE)
    a["position"][:len(pos)], a["cigar"][:len(pos)] = pos, cig
    a["flags"][len(pos) - 1] = 16
    if len(chr_end) > 1:           # a contig with no features at all: the last one
        a["position"][len(pos):] = int(chr_end[-2]) + pad + 50
        a["cigar"][len(pos):] = b"80M"
    else:
        a["position"][len(pos):] = pad + 5000
        a["cigar"][len(pos):] = b"80M"
    # the last record: 300 bases before the end of the last contig with features, an M that runs 4,700 bases past the
    # contig and 2,300 past chro_possible_length (the clamps of :1602-1603), over the two features of tail_features
    cc, prev, ln = tail_contig(chr_end, pad)
    a["position"][-1] = prev + pad + (ln - 300) - 1
    a["cigar"][-1] = b"5000M"
    return a


def tail_contig(chr_end, pad):
    """-> (the last contig make_features gives features to, the offset before it, its length)"""
    cc = 0 if len(chr_end) == 1 else len(chr_end) - 2
    prev = int(chr_end[cc - 1]) if cc else 0
    return cc, prev, int(chr_end[cc]) - prev - 2 * pad + 16


def tail_features(chr_end, pad):
    cc, _, ln = tail_contig(chr_end, pad)
    return np.array([(cc, ln - 250, ln - 200, 900004, 0, (0, 0, 0)), (cc, ln - 100, ln - 50, 900005, 0, (0, 0, 0))], CELL_FEATURE_DTYPE)


@pytest.mark.parametrize("key", KEYS + ["chr901_full"])
def test_gpu_cell_assign_records_crafted(key, open_index):
    """positions in the leading padding, at the last base before the next contig's, beyond the last
    contig; N and D; an S behind the first M (no head clip); an M past chro_possible_length; a contig
    without features"""
    ix, chr_end, pad = open_index(key)
    rng = np.random.default_rng(11)
    feats = np.concatenate([make_features(chr_end, pad, rng, per_kb=2.0),
                            np.array([(0, 990, 1010, 900001, 0, (0, 0, 0)), (0, 1300, 1330, 900002, 0, (0, 0, 0)),
                                      (0, 1005, 1100, 900003, 1, (0, 0, 0))], CELL_FEATURE_DTYPE), tail_features(chr_end, pad)])
    a = crafted(chr_end, pad)
    for allow in (0, 1):
        ix.set_cell_annotation(feats, allow_multi_overlap=allow)
        try:
            if allow:
                with pytest.raises(Exception, match="SVG_E_DEVICE"):   # 10^8 bases of M: more than 16 genes, counted, never truncated
                    ix.cell_assign_records(a)
                a = a[np.arange(len(a)) != 8]
            hits, genes = ix.cell_assign_records(a)
        finally:
            ix.set_cell_annotation(np.zeros(0, CELL_FEATURE_DTYPE))
        wh, wg = model_assign(feats, allow, chr_end, pad, a)
        assert same_hits(hits, genes, wh, wg), (key, allow)
        if allow:                  # the M past chro_possible_length gives a list, not nothing
            tail = genes[int(hits["first_gene"][-1]):][:int(hits["nhits"][-1])].tolist()
            assert hits["contig"][-1] == tail_contig(chr_end, pad)[0] and 900004 in tail and 900005 in tail
        assert hits["contig"][:5].tolist() == [-1, 0, 0, -1, -1] and hits["chro_pos"][7] == 1000 + 9 and hits["chro_pos"][6] == 1000
    h0, g0 = ix.cell_assign_records(a)           # no annotation: contig and chro_pos only
    assert (h0["nhits"] == 0).all() and len(g0) == 0 and (h0["contig"] == hits["contig"]).all() and (h0["chro_pos"] == hits["chro_pos"]).all()


def test_gpu_cell_assign_replace_on_a_live_handle(open_index, sim):
    ix, chr_end, pad = open_index(KEYS[0])
    pk, bpk = sim["pk"], sim["bpk"]
    f1 = make_features(chr_end, pad, np.random.default_rng(21), per_kb=3.0)
    f2 = make_features(chr_end, pad, np.random.default_rng(22), per_kb=3.0)
    wl2 = list(reversed(sim["wl"]))
    try:
        ix.set_cell_annotation(f1)
        ix.set_cell_barcodes(sim["wl"])
        r1 = ix.cell_assign(pk, bpk)
        ix.set_cell_annotation(f2)
        ix.set_cell_barcodes(wl2)
        r2 = ix.cell_assign(pk, bpk)
    finally:
        ix.set_cell_annotation(np.zeros(0, CELL_FEATURE_DTYPE))
        ix.set_cell_barcodes([])
    r0 = ix.cell_assign(pk, bpk)
    for r, f in ((r1, f1), (r2, f2)):
        wh, wg = model_assign(f, 0, chr_end, pad, r[1])
        assert same_hits(r[2], r[3], wh, wg)
    assert (r1[4] == sim["want_bc"]).all() and (r2[4] == model_barcodes(wl2, sim["bc"])).all()
    assert len(r1[3]) and (len(r1[3]) != len(r2[3]) or (r1[3] != r2[3]).any())
    assert len(r0[3]) == 0 and (r0[4] == -1).all() and (raw(r0[1]) == raw(ix.cell_align(pk)[1])).all()


def test_gpu_cell_assign_refusals(open_index, index_cache, sim):
    import subread_amd as sa
    ix, chr_end, pad = open_index(KEYS[0])
    for wl in ([b"ACGT", b"ACG"], [b"ACGN", b"ACGT"], [b"A" * 17], [b"ACGT", b"ACGT"]):
        with pytest.raises(sa.SvgError, match="SVG_E_ARG"):
            ix.set_cell_barcodes(wl)
    with pytest.raises(sa.SvgError, match="SVG_E_ARG"):
        ix.set_cell_annotation(np.array([(len(chr_end), 10, 20, 0, 0, (0, 0, 0))], CELL_FEATURE_DTYPE))
    ix.set_cell_barcodes(sim["wl"])
    try:
        with pytest.raises(sa.SvgError, match="SVG_E_ARG"):
            ix.cell_assign(sim["pk"], pack_barcodes(sim["bc"][:100]))
    finally:
        ix.set_cell_barcodes([])
    multi = sa.VoteIndex(index_cache.get("synth4242_fullM1"), device=0)
    try:
        with pytest.raises(sa.SvgError, match="SVG_E_UNSUPPORTED"):
            multi.cell_assign(sim["pk"])
        with pytest.raises(sa.SvgError, match="SVG_E_UNSUPPORTED"):
            multi.set_cell_annotation(np.array([(0, 10, 20, 0, 0, (0, 0, 0))], CELL_FEATURE_DTYPE))
        with pytest.raises(sa.SvgError, match="SVG_E_UNSUPPORTED"):
            multi.cell_assign_records(np.zeros(1, CELL_ALN_DTYPE))
    finally:
        multi.close()


def test_gpu_cell_assign_timing(open_index, sim):
    ix, chr_end, pad = open_index(KEYS[0])
    ix.set_cell_annotation(make_features(chr_end, pad, np.random.default_rng(5)))
    ix.set_cell_barcodes(sim["wl"])
    ix.set_timing(True)
    try:
        ix.cell_assign_timing()
        ix.cell_assign(sim["pk"], sim["bpk"])
        t = ix.cell_assign_timing()
    finally:
        ix.set_timing(False)
        ix.set_cell_annotation(np.zeros(0, CELL_FEATURE_DTYPE))
        ix.set_cell_barcodes([])
    assert set(t) == {"assign", "barcode", "scan_compact"} and all(v > 0 for v in t.values())
    assert all(v == 0 for v in ix.cell_assign_timing().values())
