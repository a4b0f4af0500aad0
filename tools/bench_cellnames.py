#!/usr/bin/env python3
"""svg_cell_count_names_batch beside svg_cell_count_batch (GPU box), both without a per-read result,
in one process: the workload of tools/bench_cellcount.py (100-base simulated reads on the C3
genome's full one-block index, its annotation, whitelist and UMIs) with BCL-style read names
composed around every read's barcode and UMI, over a sheet of 8 rows, half of them dual-index.  For
the record only: nothing is gated by it.

  bench_cellnames.py [reads (default 4,194,304)] [timed repetitions (default 3)]

One warm-up call of each, then the median of the timed calls (wall clock around the synchronous entry
points) into a reset counter.  Then one count_names_batch under svg_set_timing for the parse kernel's
own milliseconds (HIP events, summed over the chunks).  Then the plain-C model
(tests/native/cellname_model.c) parsing and packing the same names on 16 host threads: what a caller
of count_batch pays today.  The count tables and tallies of the two paths are compared.  Prints one
JSON object."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import subread_amd as sa  # noqa: E402
from subread_amd.abi import CELL_LANE_ALL, CELL_NAMES_BCL, ReadBatch  # noqa: E402
from subread_amd.sim import random_genome, c3_lengths, simulate_reads  # noqa: E402
from bench_cellassign import ACGT, ANNOT, WHITELIST, annotation  # noqa: E402
from bench_cellcount import UMI  # noqa: E402

SHEET = [(CELL_LANE_ALL, 1, b"ACGTACGT"), (CELL_LANE_ALL, 2, b"TTGGCCAA"), (1, 3, b"GGATCCAA"), (2, 4, b"CATCATCA"),
         (CELL_LANE_ALL, 5, b"GATTACAGCTTACAGA"), (CELL_LANE_ALL, 6, b"CATGCATGCAGTCAGT"), (1, 7, b"GGGGGGGGTTTTTTTT"), (2, 8, b"AACCAACCGGTTGGTT")]


def compose_names(bc, umis, rng):
    """"R%011d:" + barcode + UMI | qualities | index | qualities |@RgLater@L%03d, as a fixed-width byte matrix per index length"""
    n = len(bc)
    row = rng.integers(0, len(SHEET), n)
    lane = rng.integers(1, 3, n)
    parts, order = [], []
    for L in (8, 16):
        sel = np.flatnonzero(np.array([len(SHEET[r][2]) for r in row]) == L)
        idx = np.array([np.frombuffer(s[2], np.uint8) for s in SHEET if len(s[2]) == L])[
            np.searchsorted([i for i, s in enumerate(SHEET) if len(s[2]) == L], row[sel])]
        sub = np.flatnonzero(rng.random(len(sel)) < 0.1)
        idx[sub, rng.integers(0, L, len(sub))] = ACGT[rng.integers(0, 4, len(sub))]
        w = 13 + 28 + 1 + 28 + 1 + L + 1 + L + 14
        m = np.full((len(sel), w), ord("F"), np.uint8)
        m[:, 0] = ord("R")
        digits = (sel[:, None] // 10 ** np.arange(10, -1, -1)) % 10
        m[:, 1:12] = digits + ord("0")
        m[:, 12] = ord(":")
        m[:, 13:29], m[:, 29:41] = bc[sel], umis[sel]
        m[:, 41] = m[:, 70] = m[:, 71 + L] = ord("|")
        m[:, 71:71 + L] = idx
        tail = 72 + 2 * L
        m[:, tail:tail + 11] = np.frombuffer(b"|@RgLater@L", np.uint8)
        m[:, tail + 11:tail + 13] = ord("0")
        m[:, tail + 13] = ord("0") + lane[sel]
        parts.append(m)
        order.append(sel)
    lens = np.zeros(n, np.uint16)
    for m, sel in zip(parts, order):
        lens[sel] = m.shape[1]
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    text = np.zeros(int(lens.astype(np.int64).sum()), np.uint8)
    for m, sel in zip(parts, order):
        at = offs[sel].astype(np.int64)[:, None] + np.arange(m.shape[1])
        text[at] = m
    return ReadBatch(text, offs, lens)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4 << 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    g = random_genome(c3_lengths(), 3000, repeats=(1_000_000, 300, 200, 0.12))
    reads = simulate_reads(g, n, 100, threads=16)
    pk = sa.pack_reads(reads, threads=16)
    ix = sa.VoteIndex.build_genome(g, gap=1, memory_mb=8000, force_one_block=True, device=0)
    index = ix.export()
    chr_end, pad = index["chr_end"][:index["n_chr"]].copy(), int(index["padding"])
    del index
    feats = annotation(chr_end, pad)
    rng = np.random.default_rng(WHITELIST["seed"])
    L = WHITELIST["length"]
    wl = np.unique(ACGT[rng.integers(0, 4, (WHITELIST["barcodes"] + 4096, L))], axis=0)
    wl = wl[rng.permutation(len(wl))[:WHITELIST["barcodes"]]]
    bc = wl[rng.integers(0, len(wl), n)].copy()
    sub = np.flatnonzero(rng.random(n) < 0.25)
    bc[sub, rng.integers(0, L, len(sub))] = ACGT[rng.integers(0, 4, len(sub))]
    rng = np.random.default_rng(UMI["seed"])
    U = UMI["length"]
    umis = ACGT[rng.integers(0, 4, (UMI["molecules"], U))][rng.integers(0, UMI["molecules"], n)]
    sub = np.flatnonzero(rng.random(n) < UMI["substituted"])
    umis[sub, rng.integers(0, U, len(sub))] = ACGT[rng.integers(0, 4, len(sub))]
    assert L == 16 and U == 12
    names = compose_names(bc, umis, np.random.default_rng(1955))
    ix.set_cell_annotation(feats)
    ix.set_cell_barcodes([r.tobytes() for r in wl])
    ix.set_cell_samples(SHEET, [], 8)
    # what a caller pays today: the model on 16 threads, then count_batch
    # (the C call alone is timed, into output arrays that exist and have been written before: no allocation, page fault
    # or Python copy inside the clock; one warm-up call)
    from tests.cellname_common import model_lib, model_parse, row_text_array
    M = model_lib()
    rl, rs = np.array([r[0] for r in SHEET], np.int32), np.array([r[1] for r in SHEET], np.int32)
    rt, no_lines = row_text_array(SHEET), np.zeros(1, np.int32)
    out5, pw = np.ones((n, 5), np.int32), np.ones((n, 6), np.uint32)
    tm = []
    for i in range(reps + 1):
        t = time.perf_counter()
        M.cellname_parse_batch(names.seq.ctypes.data, names.offsets.ctypes.data, names.lens.ctypes.data, n, 1, L, U, len(SHEET), rl.ctypes.data,
                               rs.ctypes.data, rt.ctypes.data, 0, no_lines.ctypes.data, out5.ctypes.data, pw.ctypes.data, None, None, 16)
        if i:
            tm.append(time.perf_counter() - t)
    m = {"status": out5[:, 4], "sample_no": out5[:, 3].copy()}
    assert (m["status"] == 0).all()
    small = model_parse(None, CELL_NAMES_BCL, L, U, rows=SHEET, lines=[], joined=(names.seq, names.offsets[:5000], names.lens[:5000]))
    assert (small["packed"] == pw[:5000]).all() and (small["sample_no"] == m["sample_no"][:5000]).all()
    bpk = sa.abi.PackedBatch(pw[:, 0:2].reshape(-1).copy(), pw[:, 2].copy(), None, 32, np.full(n, L, np.uint16))
    upk = sa.abi.PackedBatch(pw[:, 3:5].reshape(-1).copy(), pw[:, 5].copy(), None, 32, np.full(n, U, np.uint16))
    a, b = ix.cell_counter(U, 8), ix.cell_counter(U, 8)
    a.count_names_batch(pk, names, CELL_NAMES_BCL)
    b.count_batch(pk, bpk, upk, m["sample_no"])
    tn, tc = [], []
    for _ in range(reps):
        a.reset(), b.reset()
        t = time.perf_counter()
        a.count_names_batch(pk, names, CELL_NAMES_BCL)
        tn.append(time.perf_counter() - t)
        t = time.perf_counter()
        b.count_batch(pk, bpk, upk, m["sample_no"])
        tc.append(time.perf_counter() - t)
    ra, rb, ta, tb = a.finish(), b.finish(), a.tallies(), b.tallies()
    same = bool(ra["counts"].tobytes() == rb["counts"].tobytes() and (ra["removed_umis"] == rb["removed_umis"]).all() and
                all((ta[k] == tb[k]).all() for k in ta))
    ix.set_timing(True)
    ix.cell_names_timing()
    a.reset()
    a.count_names_batch(pk, names, CELL_NAMES_BCL)
    parse_ms = ix.cell_names_timing()
    ix.set_timing(False)
    a.close(), b.close(), ix.close()
    sn, sc, sm = float(np.median(tn)), float(np.median(tc)), float(np.median(tm))
    print(json.dumps({"reads": n, "read_length": 100, "index": "C3 full one-block", "annotation": dict(ANNOT, features=len(feats)),
                      "whitelist": WHITELIST, "umi": UMI, "sheet_rows": len(SHEET), "dual_rows": sum(len(s[2]) > 12 for s in SHEET),
                      "name_bytes_per_read": round(len(names.seq) / n, 1), "timed_calls_each": reps, "statistic": "median, one process, one machine",
                      "count_names_batch_no_result_mreads_per_s": round(n / sn / 1e6, 3), "count_names_batch_seconds": [round(x, 4) for x in tn],
                      "count_batch_no_result_mreads_per_s": round(n / sc / 1e6, 3), "count_batch_seconds": [round(x, 4) for x in tc],
                      "parse_kernel_ms_one_call": round(parse_ms, 3), "parse_kernel_ns_per_read": round(parse_ms * 1e6 / n, 3),
                      "host_model_16_threads_seconds": [round(x, 4) for x in tm], "host_model_16_threads_mreads_per_s": round(n / sm / 1e6, 3),
                      "host_model_plus_count_batch_mreads_per_s": round(n / (sm + sc) / 1e6, 3),
                      "reads_with_a_sample": int((m["sample_no"] > 0).sum()), "count_table_rows": int(len(ra["counts"])),
                      "tallies": {k: [int(x) for x in v] for k, v in ta.items()}, "paths_equal": same}), flush=True)


if __name__ == "__main__":
    main()
