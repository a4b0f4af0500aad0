#!/usr/bin/env python3
"""svg_cell_assign_batch throughput (GPU box), beside svg_cell_align_batch on the same reads in
the same process: 100-base simulated reads on the C3 genome's full one-block index, 10 subreads, a
seeded synthetic annotation at the scale of a human one and a seeded whitelist of 737,000 16-base
barcodes, host buffers in and out (VoteIndex.cell_assign / VoteIndex.cell_align).  For the record
only: nothing is gated by it.

  bench_cellassign.py [reads (default 4,194,304)] [timed repetitions (default 3)]

One warm-up call of each, then the median of the timed calls (wall clock around the synchronous
entry points), alternating the two.  Then one more cell_assign call under svg_set_timing for the
per-kernel milliseconds (HIP events around each launch, summed over the chunks).  Then the plain-C
model (tests/native/cellassign_model.c) alone over the same records and barcodes on 16 threads, its
tables built once before: the host-side figure; every hit record, gene list and barcode number of
the GPU is compared with it.  Prints one JSON object."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import subread_amd as sa  # noqa: E402
from subread_amd.abi import CELL_FEATURE_DTYPE, ReadBatch  # noqa: E402
from subread_amd.sim import random_genome, c3_lengths, simulate_reads  # noqa: E402
from subread_amd.abi import CELL_HIT_DTYPE  # noqa: E402

ANNOT = dict(seed=2061, exons=300_000, exons_per_gene=10, min_len=50, max_len=400)
WHITELIST = dict(seed=1701, barcodes=737_000, length=16)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def load_model():
    """the plain-C model (tests/native/cellassign_model.c) with the host builder, built into a temporary directory"""
    import ctypes
    import subprocess
    import tempfile
    so = os.path.join(tempfile.mkdtemp(prefix="cellassign_model"), "cellassign_model.so")
    subprocess.run(["gcc", "-std=gnu11", "-O2", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", so,
                    os.path.join(ROOT, "tests", "native", "cellassign_model.c"),
                    os.path.join(ROOT, "subread_amd", "csrc", "svg_cell_annot.c"), "-lm"], check=True)
    L = ctypes.CDLL(so)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.cellassign_model_annot_new.restype = vp
    L.cellassign_model_annot_new.argtypes = [vp, u64, vp, u32, i32]
    L.cellassign_model_annot_free.argtypes = [vp]
    L.cellassign_model.restype = ctypes.c_int64
    L.cellassign_model.argtypes = [vp, i32, i32, vp, u32, i32, vp, u64, vp, vp, u64]
    L.cellassign_model_bcodes_new.restype = vp
    L.cellassign_model_bcodes_new.argtypes = [vp, u64, i32]
    L.cellassign_model_bcodes_run.restype = None
    L.cellassign_model_bcodes_run.argtypes = [vp, vp, vp, u64, vp]
    L.cellassign_model_bcodes_free.argtypes = [vp]
    return L


def annotation(chr_end, padding):
    """ANNOT["exons"] exons spread over the contigs by length, genes of exons_per_gene exons in file order"""
    rng = np.random.default_rng(ANNOT["seed"])
    lens = np.diff(np.r_[0, np.asarray(chr_end, np.int64)]) - 2 * padding + 16
    per = np.maximum(1, (ANNOT["exons"] * lens / lens.sum()).astype(np.int64))
    f = np.zeros(int(per.sum()), CELL_FEATURE_DTYPE)
    at = 0
    for c, (ln, k) in enumerate(zip(lens, per)):
        s = rng.integers(1, max(2, ln - ANNOT["max_len"]), k)
        f["contig"][at:at + k], f["start"][at:at + k] = c, s
        f["end"][at:at + k] = s + rng.integers(ANNOT["min_len"], ANNOT["max_len"], k)
        at += k
    f["gene"] = np.arange(len(f)) // ANNOT["exons_per_gene"]
    f["is_negative_strand"] = rng.integers(0, 2, len(f))
    return f


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
    # read barcodes: a whitelist entry; one read in four with a substitution, one in 64 with an N
    bc = wl[rng.integers(0, len(wl), n)].copy()
    sub = np.flatnonzero(rng.random(n) < 0.25)
    bc[sub, rng.integers(0, L, len(sub))] = ACGT[rng.integers(0, 4, len(sub))]
    nn = np.flatnonzero(rng.random(n) < 1 / 64)
    bc[nn, rng.integers(0, L, len(nn))] = ord("N")
    bpk = sa.pack_reads(ReadBatch.fixed(bc), threads=16)
    wl_list = [r.tobytes() for r in wl]
    t = time.perf_counter()
    ix.set_cell_annotation(feats)
    t_annot = time.perf_counter() - t
    t = time.perf_counter()
    ix.set_cell_barcodes(wl_list)
    t_wl = time.perf_counter() - t
    heads, alns, hits, genes, bcno = ix.cell_assign(pk, bpk)
    ix.cell_align(pk)
    ts, ta = [], []
    for _ in range(reps):
        t = time.perf_counter()
        ix.cell_assign(pk, bpk)
        ts.append(time.perf_counter() - t)
        t = time.perf_counter()
        ix.cell_align(pk)
        ta.append(time.perf_counter() - t)
    ix.set_timing(True)
    ix.cell_align_timing()
    ix.cell_assign_timing()
    ix.cell_assign(pk, bpk)
    kernels = {k: round(v, 3) for k, v in ix.cell_align_timing().items()}
    kernels.update({"assign_" + k: round(v, 3) for k, v in ix.cell_assign_timing().items()})
    ix.set_timing(False)
    ix.close()
    # the host-side figure: the plain-C model of the assignment and of the barcode rule alone, over the same records and
    # barcodes, cut into 16 ranges on 16 threads (ctypes releases the interpreter lock around the calls); the model's
    # tables are built once, outside the timed region, as the library's are by the two set calls
    from concurrent.futures import ThreadPoolExecutor
    lib = load_model()
    ce = np.ascontiguousarray(chr_end, dtype=np.uint32)
    t = time.perf_counter()
    annot = lib.cellassign_model_annot_new(feats.ctypes.data, len(feats), ce.ctypes.data, len(ce), pad)
    t_model_annot = time.perf_counter() - t
    mhits = np.zeros(len(alns), CELL_HIT_DTYPE)
    mgenes = [None] * 16
    cut = np.linspace(0, len(alns), 17).astype(np.int64)

    def assign_range(i):
        a0, a1 = int(cut[i]), int(cut[i + 1])
        g = np.zeros(max(1, (a1 - a0) * 16), np.int32)
        k = lib.cellassign_model(annot, 0, 0, ce.ctypes.data, len(ce), pad, alns[a0:a1].ctypes.data, a1 - a0, mhits[a0:a1].ctypes.data,
                                 g.ctypes.data, len(g))
        assert k >= 0
        mgenes[i] = g[:k]

    t = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(assign_range, range(16)))
    t_model_assign = time.perf_counter() - t
    lib.cellassign_model_annot_free(annot)
    # (each range numbers its genes from 0: put the ranges' lists one behind the other)
    base = 0
    for i in range(16):
        seg = mhits[int(cut[i]):int(cut[i + 1])]
        seg["first_gene"][seg["nhits"] > 0] += base
        base += len(mgenes[i])
    mg = np.concatenate(mgenes)
    cutb = np.linspace(0, n, 17).astype(np.int64)
    texts = np.zeros((n, L + 1), np.uint8)
    texts[:, :L] = bc
    wtext = np.zeros((len(wl), L + 1), np.uint8)
    wtext[:, :L] = wl
    outb = np.zeros(n, np.int32)
    t = time.perf_counter()
    bt = lib.cellassign_model_bcodes_new(wtext.ctypes.data, len(wl), L)
    t_model_wl = time.perf_counter() - t
    t = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda i: lib.cellassign_model_bcodes_run(bt, wtext.ctypes.data, texts[cutb[i]:].ctypes.data, int(cutb[i + 1] - cutb[i]),
                                                              outb[cutb[i]:].ctypes.data), range(16)))
    t_model_bc = time.perf_counter() - t
    lib.cellassign_model_bcodes_free(bt)
    same = bool((mhits.view(np.uint8) == hits.view(np.uint8)).all() and len(mg) == len(genes) and (mg == genes).all() and (outb == bcno).all())
    s, a = float(np.median(ts)), float(np.median(ta))
    new = sum(v for q, v in kernels.items() if q.startswith("assign_"))
    print(json.dumps({"reads": n, "read_length": 100, "total_subreads": 10, "index": "C3 full one-block",
                      "annotation": dict(ANNOT, features=len(feats)), "whitelist": WHITELIST,
                      "set_annotation_seconds": round(t_annot, 3), "set_barcodes_seconds": round(t_wl, 3),
                      "cell_assign_mreads_per_s": round(n / s / 1e6, 3), "cell_assign_seconds": [round(x, 4) for x in ts],
                      "cell_align_mreads_per_s": round(n / a / 1e6, 3), "cell_align_seconds": [round(x, 4) for x in ta],
                      "host_model_16_threads_seconds": {"assignment": round(t_model_assign, 4), "barcodes": round(t_model_bc, 4),
                                                        "tables_built_once_before": {"annotation": round(t_model_annot, 4),
                                                                                     "whitelist": round(t_model_wl, 4)}},
                      "kernel_ms": kernels, "new_kernels_share_of_kernel_time": round(new / sum(kernels.values()), 4),
                      "records_per_read": round(len(alns) / n, 4), "assigned_records": int((hits["nhits"] > 0).sum()),
                      "barcodes_resolved": int((bcno >= 0).sum()),
                      "bytes_back_per_read": {"cell_assign": round((heads.nbytes + alns.nbytes + hits.nbytes + genes.nbytes + bcno.nbytes) / n, 1),
                                              "cell_align": round((heads.nbytes + alns.nbytes) / n, 1)},
                      "gpu_equals_model_all_reads": same}), flush=True)


if __name__ == "__main__":
    main()
