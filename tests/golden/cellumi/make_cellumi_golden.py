#!/usr/bin/env python3
"""Generates tests/golden/cellumi/cellumi.npz with the REFERENCE's own UMI stage: ref_cellumi.c
(beside this file) #includes the reference's cell-counts.c and puts the observations of every case
through ADD_key_struct, cellCounts_do_one_batch_tab_to_struct_list, ArrayListSort with the
reference's comparator and both calls of cellCounts_do_one_batch_UMI_merge_one_step.  Needs the
reference objects under oracle/_ref/obj (make -C oracle ref), so this runs only where the reference
sources are.

Cases (tests/cellumi_common.py FIXTURE_CASES, make_case): UMI lengths 4, 11, 12 and 14, two samples,
cells including -1, sample 0, gene lists of 1 and 3 genes, and the crafted classes listed there; the
section of a few thousand entries is in the case of length 12 only (the file stays under 1 MB).

Per case the file holds the observations and, built from the reference's dump alone, the entries in
the order after the reference's first sort (CELL_UMI_ENTRY_DTYPE), the count table sorted by (sample,
cell, gene) and removed_UMIs per sample.  The outcome of an entry is read from the dump: merged =
cellbc -1 after step 1; counted = cellbc still set after step 2; of the others, the first of its
(cell, UMI) run in the list after the second sort is the removed one, the rest are lost.  The
acceptor's UMI is the value filtered_CGU_table holds under the merged entry's key; the key holds no
cell (cell-counts.c:3581-3587), so where another cell's entry took it the acceptor is recorded as
unknown (acceptor_known 0) and the tests skip that field there.  The maker asserts the class counts
from the reference's dump."""
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
from subread_amd import abi  # noqa: E402
from tests.cellumi_common import FIXTURE_CASES, N_SAMPLES, case_name, class_counts, make_case  # noqa: E402

REF_SRC = os.environ.get("REF", "/root/reference") + "/src"   # (as make_cellvote_golden.py)
DUMP = np.dtype([("cell0", "<i4"), ("gene", "<i8"), ("umi", "S14"), ("supp0", "<i4"), ("cell1", "<i4"), ("supp1", "<i4"),
                 ("acceptor", "<i4"), ("rank2", "<i4"), ("cell2", "<i4")])
CLASS_BAR = 20


def build_harness(d):
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    refcc = shlex.split(re.search(r"^REFCC\s*:=\s*(.*)$", mk, re.M).group(1))
    libs = re.search(r"^REFLIBS\s*:=\s*((?:.*\\\n)*.*)$", mk, re.M).group(1).replace("\\\n", " ").split()
    objs = [os.path.join(ROOT, "oracle", "_ref", "obj", x + ".o") for x in libs]
    assert all(os.path.exists(o) for o in objs), "build oracle/_ref first (make -C oracle ref)"
    exe = os.path.join(d, "ref-cellumi")
    subprocess.run(refcc + ["-I" + REF_SRC, '-DREF_CELL_COUNTS="%s/cell-counts.c"' % REF_SRC, "-o", exe,
                            os.path.join(HERE, "ref_cellumi.c")] + objs + ["-pthread", "-lz", "-lm"], check=True)
    return exe


def entries_of(dump, sample, L):
    d = dump[dump["cell0"] >= 0]                      # cell -1 sorts first and is skipped by both steps (:3658)
    remap = np.full(len(dump), -1)
    remap[np.nonzero(dump["cell0"] >= 0)[0]] = np.arange(len(d))
    e = np.zeros(len(d), abi.CELL_UMI_ENTRY_DTYPE)
    e["sample"], e["cell"], e["gene"], e["umi"] = sample, d["cell0"], d["gene"], d["umi"]
    e["support"], e["support_merged"] = d["supp0"], d["supp1"]
    merged = d["cell1"] < 0
    counted = ~merged & (d["cell2"] >= 0)
    e["outcome"] = np.where(merged, abi.CELL_UMI_MERGED, np.where(counted, abi.CELL_UMI_COUNTED, abi.CELL_UMI_LOST))
    # the list after the second sort: the first of a (cell, UMI) run that is not counted is the removed one
    alive = np.nonzero(~merged)[0]
    alive = alive[np.argsort(d["rank2"][alive])]
    prev = None
    for i in alive:
        k = (int(d["cell0"][i]), bytes(d["umi"][i]))
        if k != prev and not counted[i]:
            e["outcome"][i] = abi.CELL_UMI_REMOVED
        prev = k
    known = np.ones(len(d), bool)
    for i in np.nonzero(merged)[0]:
        a = int(d["acceptor"][i])
        assert a != -1, "a merged entry without a key in filtered_CGU_table"
        if a < 0:
            known[i] = False
        else:
            e["acceptor_umi"][i] = d["umi"][remap[a]] if remap[a] >= 0 else b""
    return e, known


def main():
    out, total = {}, {}
    with tempfile.TemporaryDirectory() as d:
        exe = build_harness(d)
        for L, big in FIXTURE_CASES:
            sample, cell, gene, umi = make_case(L, big, 3951 + L)
            fin, pre = os.path.join(d, "in.bin"), os.path.join(d, "out")
            with open(fin, "wb") as f:
                f.write(np.array([L, N_SAMPLES, len(sample)], np.int32).tobytes() + sample.tobytes() + cell.tobytes() + gene.tobytes() + umi.tobytes())
            subprocess.run([exe, fin, pre], check=True, stdout=subprocess.DEVNULL)
            ents, knowns, counts, removed = [], [], [], []
            for s in range(1, N_SAMPLES + 1):
                dump = np.fromfile("%s.s%d.entries" % (pre, s), DUMP)
                e, k = entries_of(dump, s, L)
                ents.append(e), knowns.append(k)
                c = np.fromfile("%s.s%d.counts" % (pre, s), np.int64).reshape(-1, 3)
                c = c[np.lexsort((c[:, 1], c[:, 0]))]
                cc = np.zeros(len(c), abi.CELL_COUNT_DTYPE)
                cc["sample"], cc["cell"], cc["gene"], cc["n_umis"] = s, c[:, 0], c[:, 1], c[:, 2]
                counts.append(cc)
                removed.append(int(np.fromfile("%s.s%d.removed" % (pre, s), np.int64)[0]))
            ent, known = np.concatenate(ents), np.concatenate(knowns)
            q = case_name(L) + "_"
            out[q + "sample"], out[q + "cell"], out[q + "gene"], out[q + "umi"] = sample.astype(np.int8), cell, gene.astype(np.int32), umi.reshape(-1)
            out[q + "entries"], out[q + "counts"] = ent.view(np.uint8), np.concatenate(counts).view(np.uint8)
            out[q + "removed"], out[q + "acceptor_known"] = np.array(removed, np.int64), known.astype(np.uint8)
            cls = class_counts(ent, L)
            print(case_name(L), "observations", len(sample), "entries", len(ent), "acceptor unknown", int((~known).sum()), "removed", removed, cls)
            for k, v in cls.items():
                total[k] = total.get(k, 0) + v
    print("classes over the cases:", total)
    for k, v in total.items():
        assert v >= (1 if k == "thousands" else CLASS_BAR), (k, v)
    path = os.path.join(HERE, "cellumi.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
