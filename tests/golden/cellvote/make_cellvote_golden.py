#!/usr/bin/env python3
"""Generates tests/golden/cellvote/cellvote.npz with the REFERENCE's own cellCounts voting step:
ref_cellvote.c (beside this file) #includes the reference's cell-counts.c and runs its
prefill_votes and cellCounts_process_copy_ptrs_to_votes per read.  The harness is compiled into a
temporary directory with oracle/Makefile's REFCC flags against the reference objects under
oracle/_ref/obj (make -C oracle ref), so this runs only where the reference sources are.

One case per (index, total_subreads): chr901_full, chr901_gapped, synth4242_full,
synth4242_gapped x 7, 10, 20.  The 320 reads of a case: lengths 16, 17, 18, 19, 31, 50, 100, 160
in turn (the indel and chimeric classes: 50, 100, 160 only), either strand, of ten classes in
turn: exact; 1% substitutions; one 1-5 base insertion; one such deletion; N bases; reads that
begin with a 16-mer of one of the index's longest hit lists (more than 64 items where the index
has such lists, else more than half of its longest) -- the repeat families of synth4242, the
repeats of chr901; reads from 16-mers of more than 8 hits with an insertion, and with a deletion;
chimeric reads whose second half is the reverse complement of another place (slots of both
strands in one table), plain and from repeats.  A few reads under 16 bases are among them.

Every key the harness looked up is checked against a numpy genekey2int of the read text (of its
reverse complement for strand 1) at that offset.  Stored per case: the packed reads
(svg_packed_reads: bases, xmask, starts, lens), the expected heads and slots (svg_cell_head /
svg_cell_slot bytes) and each read's longest hit list (max_run)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
from tests.common import IndexCache, revcomp_bytes  # noqa: E402
from tests.cellvote_common import CASES, edge_counts, host_index, index_runs, long_run_bar  # noqa: E402
from subread_amd.abi import CELL_HEAD_DTYPE, CELL_SLOT_DTYPE, PackedBatch, ReadBatch  # noqa: E402
from subread_amd.sim import Genome  # noqa: E402

REF_SRC = os.environ.get("REF", "/root/reference") + "/src"
LENGTHS = (16, 17, 18, 19, 31, 50, 100, 160)
READS = 320
ACGT = np.frombuffer(b"ACGT", np.uint8)
CODE = np.full(256, 3, np.uint32)
CODE[:ord("G")] = 2
CODE[ord("A")], CODE[ord("G")] = 0, 1   # base2int, subread.h:238


def build_harness(d):
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    refcc = re.search(r"^REFCC\s*:=\s*(.*)$", mk, re.M).group(1)   # (shlex turns its \" into the shell's literal quote)
    libs = re.search(r"^REFLIBS\s*:=\s*((?:.*\\\n)*.*)$", mk, re.M).group(1).replace("\\\n", " ").split()
    objs = [os.path.join(ROOT, "oracle", "_ref", "obj", x + ".o") for x in libs]
    assert all(os.path.exists(o) for o in objs), "build oracle/_ref first (make -C oracle ref)"
    exe = os.path.join(d, "ref-cellvote")
    import shlex
    cmd = shlex.split(refcc) + ["-I" + REF_SRC, '-DREF_CELL_COUNTS="%s/cell-counts.c"' % REF_SRC, "-o", exe,
                                os.path.join(HERE, "ref_cellvote.c")] + objs + ["-pthread", "-lz", "-lm"]
    subprocess.run(cmd, check=True)
    return exe


def genome_kmers(flat):
    """genekey2int of the 16-mer at every position of the genome"""
    k = np.zeros(len(flat) - 15, np.uint64)
    for i in range(16):
        k = (k << np.uint64(2)) | CODE[flat[i:len(flat) - 15 + i]].astype(np.uint64)
    return k


def hot_positions(kmers, ix):
    """genome positions whose 16-mer has one of the index's longest hit lists (more than 64 items
    where the index has such lists, else more than half of its longest), and those with more than 8"""
    key, length = index_runs(ix)
    top = long_run_bar(int(length.max()))
    return (np.flatnonzero(np.isin(kmers, key[length > top])), np.flatnonzero(np.isin(kmers, key[length > 8])),
            int(length.max()))


# class of read i (i // 8 % 10); the indel and chimeric classes take no length under 50
EXACT, SUBST, INS, DEL, NBASE, HOT, WARM_INS, WARM_DEL, CHIMERA, HOT_CHIMERA = range(10)


def make_reads(g, hot, warm, rng):
    f = g.flat

    def place(src, L):
        if src is not None and len(src):
            # a subread starts at offset 0 of either strand: the repeated 16-mer first
            return min(max(int(src[rng.integers(0, len(src))]), 0), len(f) - L - 8)
        return int(rng.integers(0, len(f) - L - 8))

    reads = []
    for i in range(READS):
        L = LENGTHS[i % len(LENGTHS)]
        cls = (i // len(LENGTHS)) % 10
        if cls in (INS, DEL, WARM_INS, WARM_DEL, CHIMERA, HOT_CHIMERA) and L < 50:
            L = (50, 100, 160, 100, 160)[i % 5] if cls < CHIMERA else (100, 160)[i % 2]
        if i % 61 == 60:
            L, cls = int(rng.integers(0, 16)), EXACT    # skipped by the reference (cell-counts.c:3077)
        src = hot if cls in (HOT, HOT_CHIMERA) else warm if cls in (WARM_INS, WARM_DEL) else None
        s = place(src, L)
        r = bytearray(f[s:s + L + 8].tobytes())
        if cls in (INS, WARM_INS):                  # insertion of 1-5 bases
            at, k = int(rng.integers(20, L - 20)), int(rng.integers(1, 6))
            r[at:at] = ACGT[rng.integers(0, 4, k)].tobytes()
        elif cls in (DEL, WARM_DEL):                # deletion of 1-5 bases
            at, k = int(rng.integers(20, L - 20)), int(rng.integers(1, 6))
            del r[at:at + k]
        r = np.frombuffer(bytes(r[:L]), np.uint8).copy()
        if cls in (CHIMERA, HOT_CHIMERA):           # second half: the reverse complement of another place
            h = L // 2
            s2 = place(warm if cls == HOT_CHIMERA else None, L - h)
            r[h:] = revcomp_bytes(f[s2:s2 + L - h])
        if cls in (SUBST, INS, DEL):
            hit = rng.random(L) < 0.01
            r[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        if cls == NBASE and L:
            r[rng.random(L) < 0.03] = ord("N")
            r[int(rng.integers(0, L))] = ord("N")
        if rng.random() < 0.5:
            r = revcomp_bytes(r)
        reads.append(r.tobytes())
    return reads


def check_keys(reads, keys):
    """every key of the harness == genekey2int (input-files.c:1232) of the text at its offset"""
    for rno, strand, off, key, _ in keys:
        t = np.frombuffer(reads[rno], np.uint8)
        if strand:
            t = revcomp_bytes(t)
        want = 0
        for c in t[off:off + 16]:
            want = (want << 2) | int(CODE[c])
        assert want == key, (rno, strand, off, key, want)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        exe = build_harness(d)
        cache = IndexCache(d)
        genomes, hots = {}, {}
        for key, total in CASES:
            gname = key.rsplit("_", 1)[0]
            pre = cache.get(key)
            if gname not in genomes:
                g = Genome.read_fasta(cache.genome_fasta(gname))
                genomes[gname] = (g, genome_kmers(g.flat))
            if key not in hots:
                hots[key] = hot_positions(genomes[gname][1], host_index(pre))
            rng = np.random.default_rng(3051 + total + 100 * CASES.index((key, total)))
            reads = make_reads(genomes[gname][0], hots[key][0], hots[key][1], rng)
            fr, fh, fs, fk = (os.path.join(d, x) for x in ("reads.txt", "heads.bin", "slots.bin", "keys.bin"))
            with open(fr, "wb") as f:
                f.write(b"".join(r + b"\n" for r in reads))
            subprocess.run([exe, pre, str(total), fr, fh, fs, fk], check=True)
            heads = np.fromfile(fh, CELL_HEAD_DTYPE)
            slots = np.fromfile(fs, CELL_SLOT_DTYPE)
            keys = np.fromfile(fk, np.uint32).reshape(-1, 5)
            assert len(heads) == len(reads) and int(heads["n_slots"].sum()) == len(slots)
            check_keys(reads, keys)
            max_run = np.zeros(len(reads), np.uint32)
            np.maximum.at(max_run, keys[:, 0], keys[:, 4])
            pk = PackedBatch.pack_numpy(ReadBatch.from_list(reads))
            p = "%s_n%d_" % (key, total)
            out[p + "bases"], out[p + "starts"], out[p + "lens"] = pk.bases, pk.starts, pk.lens
            out[p + "xmask"] = pk.xmask if pk.xmask is not None else np.zeros(0, np.uint32)
            out[p + "heads"] = heads.view(np.uint8)
            out[p + "slots"] = slots.view(np.uint8)
            out[p + "max_run"] = max_run
            print(key, total, "slots", len(slots), edge_counts(heads, slots, max_run))
    path = os.path.join(HERE, "cellvote.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
