#!/usr/bin/env python3
"""Generates tests/golden/cellassign/cellassign.npz with the REFERENCE's own annotation loader
(cellCounts_load_annotations: load_features_annotation with features_load_one_line, and
cellCounts_sort_feature_info), cellCounts_make_barcode_HT_table, cellCounts_get_cellbarcode_no and
cellCounts_write_read_in_batch_bin: ref_cellassign.c (beside this file) #includes the reference's
cell-counts.c, votes and aligns each read as ref_cellalign.c does and lets the reference's writer
run; its calls of cellCounts_vote_and_add_count land in a recorder (the harness object is compiled
-fPIC, that function weakened with objcopy, the recorder is the strong definition in a second
object).  Needs the reference objects under oracle/_ref/obj (make -C oracle ref), so this runs only
where the reference sources are.

Cases (tests/cellassign_common.py FIXTURE_CASES): synth4242_full and chr901_gapped x 7, 10, 20
subreads at the default parameters, and both at 10 subreads with the second parameter set (5
reported alignments).  allow_multi_overlapping_reads is set on the second set and at 20 subreads.
Reads of a case: those of the cellalign fixture's maker (the cellvote classes and its extra
classes: indels, soft clips, repeats), every second one of them (the file stays under 1 MB), then
80 reads drawn across the first 131,072-base bucket border and up to 36 reads placed across the
border of two feature blocks (the host builder's tables say where; the test checks them against
the reference's).  The annotation is make_features' (ties in start, features across the border, both
strands, dense enough that every class of tests/test_cellassign_golden.py is met), its genes
numbered by first appearance as the reference numbers them.  Each read gets a cell barcode of one
of the classes of make_read_barcodes_fixture.  A read for which the reference turns a call inside
its loop into an unmapped one (no chromosome) is dropped and the case run again; the count is
printed."""
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
from tests.common import IndexCache, revcomp_bytes  # noqa: E402
from tests.cellalign_common import case_params, host_index  # noqa: E402
from tests.cellassign_common import (FIXTURE_CASES, build_tables, fixture_allow, make_features, make_read_barcodes_fixture, make_whitelist_fixture,  # noqa: E402
                                     renumber_genes)
from subread_amd.abi import CELL_ALN_DTYPE, CELL_ALN_HEAD_DTYPE, CELL_HIT_DTYPE, PackedBatch, ReadBatch  # noqa: E402
from subread_amd.sim import Genome  # noqa: E402


def load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, *path))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


cv = load("make_cellvote_golden", "..", "cellvote", "make_cellvote_golden.py")
ca = load("make_cellalign_golden", "..", "cellalign", "make_cellalign_golden.py")
REF_SRC = cv.REF_SRC
PAD = 1210


def build_harness(d):
    import re
    import shlex
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    refcc = shlex.split(re.search(r"^REFCC\s*:=\s*(.*)$", mk, re.M).group(1))
    libs = re.search(r"^REFLIBS\s*:=\s*((?:.*\\\n)*.*)$", mk, re.M).group(1).replace("\\\n", " ").split()
    objs = [os.path.join(ROOT, "oracle", "_ref", "obj", x + ".o") for x in libs]
    assert all(os.path.exists(o) for o in objs), "build oracle/_ref first (make -C oracle ref)"
    src = os.path.join(HERE, "ref_cellassign.c")
    o1, o1w, o2, exe = (os.path.join(d, x) for x in ("harness.o", "harness-weak.o", "recorder.o", "ref-cellassign"))
    subprocess.run(refcc + ["-fPIC", "-I" + REF_SRC, '-DREF_CELL_COUNTS="%s/cell-counts.c"' % REF_SRC, "-c", "-o", o1, src], check=True)
    subprocess.run(["objcopy", "--weaken-symbol=cellCounts_vote_and_add_count", o1, o1w], check=True)
    subprocess.run(refcc + ["-fPIC", "-DCELLASSIGN_RECORDER", "-c", "-o", o2, src], check=True)
    subprocess.run(refcc + ["-o", exe, o1w, o2] + objs + ["-pthread", "-lz", "-lm"], check=True)
    return exe


def border_reads(g, rng):
    f = g.flat
    out = []
    for j in range(80):
        s = 131072 - 160 + 2 * j + int(rng.integers(0, 2))
        r = f[s:s + 100].copy()
        out.append((revcomp_bytes(r) if j % 2 else r).tobytes())
    return out


def block_border_reads(g, feats, chr_end, limit=36):
    """reads of contig 0 that start 50 bases before the first feature of a block whose strand is that of
    the last feature of the block before it, where that one reaches into the read: raw hits from two blocks"""
    t = build_tables(feats, chr_end, PAD)
    n0 = int(t["contigs"][1])                    # contig 0's blocks
    f, out = g.flat, []
    for b in range(1, n0):
        q = int(t["block_end"][b - 1])
        s = int(t["start"][q]) - 51
        if t["strand"][q] != t["strand"][q - 1] or int(t["stop"][q - 1]) < s + 1 or s < 0 or s + 100 > int(chr_end[0]) - 2 * PAD:
            continue
        r = f[s:s + 100].copy()
        out.append((revcomp_bytes(r) if t["strand"][q] else r).tobytes())
        if len(out) == limit:
            break
    return out


def read_tables(path):
    b = open(path, "rb").read()
    nf, nb, nc, nw = (int(x) for x in np.frombuffer(b, np.uint64, 4))
    at = 32
    out = {}
    for key, dt, n in (("start", np.int64, nf), ("stop", np.int64, nf), ("strand", np.uint8, nf), ("gene", np.int32, nf),
                       ("block_end", np.int64, nb), ("block_min", np.int64, nb), ("block_max", np.int64, nb),
                       ("contigs", np.uint32, 3 * nc), ("rev", np.uint32, nw)):
        out[key] = np.frombuffer(b, dt, n, at).copy()
        at += n * np.dtype(dt).itemsize
    assert at == len(b)
    return out


def main():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        exe = build_harness(d)
        cache = IndexCache(d)
        genomes, hots = {}, {}
        for ci, (key, total, which) in enumerate(FIXTURE_CASES):
            gname = key.rsplit("_", 1)[0]
            pre = cache.get(key)
            if gname not in genomes:
                g = Genome.read_fasta(cache.genome_fasta(gname))
                genomes[gname] = (g, cv.genome_kmers(g.flat))
            if key not in hots:
                hots[key] = cv.hot_positions(genomes[gname][1], host_index(pre))
            g = genomes[gname][0]
            rng = np.random.default_rng(2061 + total + 100 * ci)
            p = case_params(total, which)
            reads = (cv.make_reads(g, hots[key][0], hots[key][1], rng) +
                     ca.extra_reads(g, hots[key][0], hots[key][1], rng, p["max_mismatching_bases_in_reads"]))[::2] + border_reads(g, rng)
            chr_end = np.array([int(x.split("\t")[0]) for x in open(pre + ".reads").read().split("\n") if "\t" in x], np.uint32)
            feats = renumber_genes(make_features(chr_end, PAD, rng, per_kb=6.0, genes_per=3, border=24))
            reads = reads + block_border_reads(g, feats, chr_end)
            wl, xs = make_whitelist_fixture(400, 16, rng)
            bcs = make_read_barcodes_fixture(wl, xs, len(reads), rng)
            allow = fixture_allow(total, which)
            dropped = 0
            while True:
                fr, ff, fw = (os.path.join(d, x) for x in ("reads.txt", "features.bin", "whitelist.txt"))
                with open(fr, "wb") as f:
                    f.write(b"".join(r + b" " + b + b"\n" for r, b in zip(reads, bcs)))
                feats.tofile(ff)
                with open(fw, "wb") as f:
                    f.write(b"".join(w + b"\n" for w in wl))
                subprocess.run([exe, pre, fr, ff, fw, d, str(allow)] + [str(p[k]) for k in (
                    "total_subreads", "min_votes_per_mapped_read", "max_differential_from_top_vote_number",
                    "max_mismatching_bases_in_reads", "min_mapped_length_for_mapped_read", "max_reported_alignments_per_read")],
                    check=True, stdout=subprocess.DEVNULL)
                flags = np.fromfile(os.path.join(d, "flags.bin"), np.uint8)
                if not flags.any():
                    break
                dropped += int(flags.sum())
                reads = [r for r, x in zip(reads, flags) if not x]
                bcs = [b for b, x in zip(bcs, flags) if not x]
            heads = np.fromfile(os.path.join(d, "heads.bin"), CELL_ALN_HEAD_DTYPE)
            alns = np.fromfile(os.path.join(d, "alns.bin"), CELL_ALN_DTYPE)
            hits = np.fromfile(os.path.join(d, "hits.bin"), CELL_HIT_DTYPE)
            genes = np.fromfile(os.path.join(d, "genes.bin"), np.int32)
            bcno = np.fromfile(os.path.join(d, "bc.bin"), np.int32)
            t = read_tables(os.path.join(d, "tables.bin"))
            assert len(heads) == len(reads) == len(bcno) and int(heads["n_records"].sum()) == len(alns) == len(hits)
            pk = PackedBatch.pack_numpy(ReadBatch.from_list(reads))
            q = "%s_n%d_%s_" % (key, total, which)
            out[q + "bases"], out[q + "starts"], out[q + "lens"] = pk.bases, pk.starts, pk.lens
            out[q + "xmask"] = pk.xmask if pk.xmask is not None else np.zeros(0, np.uint32)
            out[q + "features"] = feats.view(np.uint8)
            out[q + "whitelist"] = np.frombuffer(b"".join(wl), np.uint8)
            out[q + "barcodes"] = np.frombuffer(b"".join(bcs), np.uint8)
            out[q + "chr_end"] = chr_end
            out[q + "heads"], out[q + "alns"] = heads.view(np.uint8), alns.view(np.uint8)
            out[q + "hits"], out[q + "genes"], out[q + "bcno"] = hits.view(np.uint8), genes, bcno
            for k, v in t.items():
                out[q + "t_" + k] = v.astype(np.uint32) if v.dtype == np.int64 else v
            print(key, total, which, "allow", allow, "reads", len(reads), "dropped", dropped, "records", len(alns),
                  "nhits 0/1/2+", int((hits["nhits"] == 0).sum()), int((hits["nhits"] == 1).sum()), int((hits["nhits"] > 1).sum()),
                  "barcodes resolved", int((bcno >= 0).sum()))
    path = os.path.join(HERE, "cellassign.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
