#!/usr/bin/env python3
"""Generates tests/golden/cellalign/cellalign.npz with the REFERENCE's own
cellCounts_select_and_write_alignments: ref_cellalign.c (beside this file) #includes the
reference's cell-counts.c, makes each read's vote table with the reference's functions and calls
the reference's function; its calls of cellCounts_write_read_in_batch_bin land in a recorder (the
harness object is compiled -fPIC, the writer weakened with objcopy, the recorder is the strong
definition in a second object -- the way oracle/Makefile replaces do_voting).  Needs the reference
objects under oracle/_ref/obj (make -C oracle ref), so this runs only where the reference sources
are.

Cases (tests/cellalign_common.py CASES): the four cellvote indexes x 7, 10, 20 subreads at the
default parameters, and synth4242_full and chr901_gapped at 10 subreads with the second parameter
set.  Reads of a case: the 320 reads of the cellvote classes (make_cellvote_golden.make_reads),
then 100-base and 160-base reads with two indels, with 6-12 mismatched bases at the head or the
tail (soft clips), from the index's repeated 16-mers (the longest hit lists, and those of more
than 8: tied scores), and with max_mismatching_bases_in_reads + 2 substitutions in the middle.  The exon list is drawn so
that about a third of the reads lie inside an exon, a third within 100 bases of one and the rest
outside both.  A read for which the model reports a candidate outside the reference's contract
(subread_vote.h: a genome base outside the .array image, the recorder's overrun) is dropped; the
count is printed."""
import importlib.util
import os
import re
import shlex
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
from tests.common import IndexCache, revcomp_bytes  # noqa: E402
from tests.cellalign_common import CASES, EDGES, case_params, host_index, make_exons, model_align, raw  # noqa: E402
from subread_amd.abi import CELL_ALN_DTYPE, CELL_ALN_HEAD_DTYPE, PackedBatch, ReadBatch  # noqa: E402
from subread_amd.sim import Genome  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_cellvote_golden", os.path.join(HERE, "..", "cellvote", "make_cellvote_golden.py"))
cv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cv)

REF_SRC = cv.REF_SRC
ACGT = cv.ACGT
EXTRA = 770


def build_harness(d):
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    refcc = shlex.split(re.search(r"^REFCC\s*:=\s*(.*)$", mk, re.M).group(1))
    libs = re.search(r"^REFLIBS\s*:=\s*((?:.*\\\n)*.*)$", mk, re.M).group(1).replace("\\\n", " ").split()
    objs = [os.path.join(ROOT, "oracle", "_ref", "obj", x + ".o") for x in libs]
    assert all(os.path.exists(o) for o in objs), "build oracle/_ref first (make -C oracle ref)"
    src = os.path.join(HERE, "ref_cellalign.c")
    o1, o1w, o2, exe = (os.path.join(d, x) for x in ("harness.o", "harness-weak.o", "recorder.o", "ref-cellalign"))
    subprocess.run(refcc + ["-fPIC", "-I" + REF_SRC, '-DREF_CELL_COUNTS="%s/cell-counts.c"' % REF_SRC, "-c", "-o", o1, src], check=True)
    subprocess.run(["objcopy", "--weaken-symbol=cellCounts_write_read_in_batch_bin", o1, o1w], check=True)
    subprocess.run(refcc + ["-fPIC", "-DCELLALIGN_RECORDER", "-c", "-o", o2, src], check=True)
    subprocess.run(refcc + ["-o", exe, o1w, o2] + objs + ["-pthread", "-lz", "-lm"], check=True)
    return exe


def extra_reads(g, hot, warm, rng, max_mm):
    f = g.flat
    reads = []
    for i in range(EXTRA):
        L = (100, 160)[i % 2]
        cls = i % 7
        src = hot if cls == 3 else warm if cls in (4, 6) else None
        s = cv_place(f, src, L, rng)
        r = bytearray(f[s:s + L + 16].tobytes())
        if cls == 0:      # two indels, 30 or more bases apart
            a1 = int(rng.integers(20, L // 2 - 15))
            a2 = int(rng.integers(L // 2 + 15, L - 20))
            for at in (a2, a1):
                k = int(rng.integers(1, 5))
                if rng.random() < 0.5:
                    r[at:at] = ACGT[rng.integers(0, 4, k)].tobytes()
                else:
                    del r[at:at + k]
        r = np.frombuffer(bytes(r[:L]), np.uint8).copy()
        if cls in (1, 2):  # 6-12 mismatched bases at the head (1) or the tail (2)
            k = int(rng.integers(6, 13))
            seg = slice(0, k) if cls == 1 else slice(L - k, L)
            r[seg] = ACGT[(np.searchsorted(ACGT, r[seg]) + rng.integers(1, 4, k)) % 4]
        if cls == 5:       # max_mm + 2 substitutions, every other base of the middle: scored 0 for its mismatches
            at = L // 2 - (max_mm + 2) + 2 * np.arange(max_mm + 2)
            r[at] = ACGT[(np.searchsorted(ACGT, r[at]) + rng.integers(1, 4, len(at))) % 4]
        if rng.random() < 0.5:
            r = revcomp_bytes(r)
        reads.append(r.tobytes())
    return reads


def cv_place(f, src, L, rng):
    if src is not None and len(src):
        return min(max(int(src[rng.integers(0, len(src))]), 0), len(f) - L - 16)
    return int(rng.integers(0, len(f) - L - 16))


def main():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        exe = build_harness(d)
        cache = IndexCache(d)
        genomes, hots, hosts = {}, {}, {}
        for ci, (key, total, which) in enumerate(CASES):
            gname = key.rsplit("_", 1)[0]
            pre = cache.get(key)
            if gname not in genomes:
                g = Genome.read_fasta(cache.genome_fasta(gname))
                genomes[gname] = (g, cv.genome_kmers(g.flat))
            if key not in hots:
                hosts[key] = host_index(pre)
                hots[key] = cv.hot_positions(genomes[gname][1], hosts[key])
            g = genomes[gname][0]
            rng = np.random.default_rng(2648 + total + 100 * ci)
            reads = cv.make_reads(g, hots[key][0], hots[key][1], rng) + extra_reads(g, hots[key][0], hots[key][1], rng, case_params(total, which)["max_mismatching_bases_in_reads"])
            ex_a, ex_b = make_exons(len(g.flat), rng)
            p = case_params(total, which)
            # reads outside the reference's contract (the model counts them) are dropped
            _, _, outside = model_align(hosts[key], ReadBatch.from_list(reads), (ex_a, ex_b), want_outside=True, **p)
            keep = [r for r, o in zip(reads, outside) if not o]
            print(key, total, which, "dropped", len(reads) - len(keep), "of", len(reads))
            reads = keep
            fr, fe, fh, fa = (os.path.join(d, x) for x in ("reads.txt", "exons.bin", "heads.bin", "alns.bin"))
            with open(fr, "wb") as f:
                f.write(b"".join(r + b"\n" for r in reads))
            np.stack([ex_a, ex_b], 1).astype(np.uint32).tofile(fe)
            subprocess.run([exe, pre, fr, fe, fh, fa] + [str(p[k]) for k in (
                "total_subreads", "min_votes_per_mapped_read", "max_differential_from_top_vote_number",
                "max_mismatching_bases_in_reads", "min_mapped_length_for_mapped_read", "max_reported_alignments_per_read")],
                check=True)
            heads = np.fromfile(fh, CELL_ALN_HEAD_DTYPE)
            alns = np.fromfile(fa, CELL_ALN_DTYPE)
            assert len(heads) == len(reads) and int(heads["n_records"].sum()) == len(alns)
            mh, ma, edges = model_align(hosts[key], ReadBatch.from_list(reads), (ex_a, ex_b), want_edges=True, **p)
            same = (raw(mh) == raw(heads)).all() and len(ma) == len(alns) and (raw(ma) == raw(alns)).all()
            pk = PackedBatch.pack_numpy(ReadBatch.from_list(reads))
            q = "%s_n%d_%s_" % (key, total, which)
            out[q + "bases"], out[q + "starts"], out[q + "lens"] = pk.bases, pk.starts, pk.lens
            out[q + "xmask"] = pk.xmask if pk.xmask is not None else np.zeros(0, np.uint32)
            out[q + "exons"] = np.stack([ex_a, ex_b], 1).astype(np.uint32).reshape(-1)
            out[q + "heads"] = raw(heads)
            out[q + "alns"] = raw(alns)
            print("   records", len(alns), "mapped reads", int((heads["n_records"] > 0).sum()), "model equal:", bool(same),
                  {k: int(((edges & v) != 0).sum()) for k, v in EDGES.items()})
    path = os.path.join(HERE, "cellalign.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
