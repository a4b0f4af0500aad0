#!/usr/bin/env python3
"""Generates tests/golden/cellname/cellname.npz with the REFERENCE's own read-name functions:
ref_cellname.c (beside this file) #includes the reference's cell-counts.c and calls
cellCounts_scan_read_name_str, cellCounts_get_sample_id, hamming_dist_ATGC_max1 and
hamming_dist_ATGC_max1_2p on the names of tests/cellname_common.py (make_names), in BCL and in FASTQ
mode.  Needs the reference objects under oracle/_ref/obj (make -C oracle ref), so it runs only where
the reference sources are.  See README.txt for what the file holds and what it does not pin."""
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
from tests.cellname_common import CLASSES, FASTQ, LINES, MODES, ROWS, class_counts, make_names, mutate, row_text_array  # noqa: E402

REF_SRC = os.environ.get("REF", "/root/reference") + "/src"   # (as make_cellvote_golden.py)
OUT = np.dtype([("fields", "<i4"), ("trimmed", "<i4"), ("lane", "<i4"), ("sample", "<i4"), ("bc", "S16"), ("umi", "S16")])
CLASS_BAR = 20


def build_harness(d):
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    refcc = shlex.split(re.search(r"^REFCC\s*:=\s*(.*)$", mk, re.M).group(1))
    libs = re.search(r"^REFLIBS\s*:=\s*((?:.*\\\n)*.*)$", mk, re.M).group(1).replace("\\\n", " ").split()
    objs = [os.path.join(ROOT, "oracle", "_ref", "obj", x + ".o") for x in libs]
    assert all(os.path.exists(o) for o in objs), "build oracle/_ref first (make -C oracle ref)"
    exe = os.path.join(d, "ref-cellname")
    subprocess.run(refcc + ["-I" + REF_SRC, '-DREF_CELL_COUNTS="%s/cell-counts.c"' % REF_SRC, "-o", exe,
                            os.path.join(HERE, "ref_cellname.c")] + objs + ["-pthread", "-lz", "-lm"], check=True)
    return exe


def make_pairs(rng, n=400):
    """pairs of texts for the two Hamming functions: equal, near, far, of unequal length, with N and with a stop character"""
    pairs = np.zeros((n, 2, 33), np.uint8)
    for i in range(n):
        L = int(rng.integers(1, 33))
        a = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)])
        b = mutate(a, rng.integers(0, L, i % 5), rng)
        if i % 7 == 0:
            b = b[:max(1, L - int(rng.integers(1, 4)))]
        if i % 11 == 0:
            a = a.replace(b"A", b"N", 1)
        if i % 13 == 0:
            a = a[:L // 2] + b"|" + a[L // 2 + 1:]
        pairs[i, 0, :len(a)] = np.frombuffer(a, np.uint8)
        pairs[i, 1, :len(b)] = np.frombuffer(b, np.uint8)
    return pairs


def main():
    out, total = {}, dict.fromkeys(CLASSES, 0)
    rows = np.zeros(len(ROWS), np.dtype([("lane", "<i4"), ("sample", "<i4"), ("index", "S33")]))
    for i, r in enumerate(ROWS):
        rows[i] = r
    pairs = make_pairs(np.random.default_rng(1072))
    with tempfile.TemporaryDirectory() as d:
        exe = build_harness(d)
        for which, (mode, bl, ul) in MODES.items():
            names = make_names(which, 1658 + mode)
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([mode, bl, ul, len(ROWS), len(LINES), len(names), len(pairs)], np.int32).tobytes())
                f.write(rows.tobytes() + np.array(LINES, np.int32).tobytes())
                for nm in names:
                    f.write(np.int32(len(nm)).tobytes() + nm)
                f.write(pairs.tobytes())
            subprocess.run([exe, fin, fout], check=True, stdout=subprocess.DEVNULL)
            raw = open(fout, "rb").read()
            ref = np.frombuffer(raw[:OUT.itemsize * len(names)], OUT)
            dist = np.frombuffer(raw[OUT.itemsize * len(names):], np.int32).reshape(-1, 2)
            assert len(dist) == len(pairs)
            offs = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.int64)
            out[which + "_text"] = np.frombuffer(b"".join(names), np.uint8)
            out[which + "_offs"] = offs
            out[which + "_ref"] = np.stack([ref["fields"], ref["trimmed"], ref["lane"], ref["sample"]], 1).astype(np.int32)
            out[which + "_bc"] = np.frombuffer(ref["bc"].tobytes(), np.uint8).reshape(-1, 16)[:, :bl].copy()
            out[which + "_umi"] = np.frombuffer(ref["umi"].tobytes(), np.uint8).reshape(-1, 16)[:, :ul].copy()
            cls = class_counts(names, mode, ref["lane"], ref["sample"])
            print(which, len(names), "names", cls)
            for k, v in cls.items():
                total[k] += v
            out["pair_dist"] = dist
    out["pairs"] = pairs
    out["rows_lane"], out["rows_sample"], out["rows_text"] = rows["lane"], rows["sample"], row_text_array()
    out["lines"] = np.array(LINES, np.int32)
    print("classes over the modes:", total)
    for k, v in total.items():
        assert v >= CLASS_BAR, (k, v)
    path = os.path.join(HERE, "cellname.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 981006


if __name__ == "__main__":
    main()
