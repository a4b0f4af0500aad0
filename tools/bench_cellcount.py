#!/usr/bin/env python3
"""svg_cell_count_batch + svg_cell_counter_finish throughput (GPU box), beside svg_cell_assign_batch
on the same reads in the same process: the workload of tools/bench_cellassign.py (100-base simulated
reads on the C3 genome's full one-block index, 10 subreads, its annotation and whitelist) with a
12-base UMI per read, drawn from 200,000 molecules' UMIs with one read in ten carrying a
substitution, and one sample.  For the record only: nothing is gated by it.

  bench_cellcount.py [reads (default 4,194,304)] [timed repetitions (default 3)]

One warm-up call of each, then the median of the timed calls (wall clock around the synchronous
entry points): count_batch without a per-read result into a reset counter, then finish, then
cell_assign.  Then one more count_batch + finish under svg_set_timing for the per-kernel
milliseconds (HIP events, summed over the chunks).  Then the plain-C model
(tests/native/cellumi_model.c) over the same observations, cut by cell into 16 parts on 16 threads:
the host-side figure; the GPU's count table is compared with it.  Prints one JSON object."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import subread_amd as sa  # noqa: E402
from subread_amd.abi import ReadBatch  # noqa: E402
from subread_amd.sim import random_genome, c3_lengths, simulate_reads  # noqa: E402
from bench_cellassign import ACGT, ANNOT, WHITELIST, annotation  # noqa: E402

UMI = dict(seed=3951, length=12, molecules=200_000, substituted=0.1)


def observations(heads, hits, genes, bcno, umis):
    """one (cell, gene, UMI) per (record, gene of its list), as svg_cell_count_batch expands them"""
    read_of = np.repeat(np.arange(len(heads)), heads["n_records"])
    ok = (hits["contig"] >= 0) & (hits["nhits"] > 0)
    k = hits["nhits"][ok].astype(np.int64)
    rec = np.repeat(np.nonzero(ok)[0], k)
    within = np.arange(len(rec)) - np.repeat(np.cumsum(k) - k, k)
    g = genes[hits["first_gene"][rec].astype(np.int64) + within]
    r = read_of[rec]
    return bcno[r].astype(np.int32), g.astype(np.int64), umis[r]


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
    bpk = sa.pack_reads(ReadBatch.fixed(bc), threads=16)
    rng = np.random.default_rng(UMI["seed"])
    U = UMI["length"]
    umis = ACGT[rng.integers(0, 4, (UMI["molecules"], U))][rng.integers(0, UMI["molecules"], n)]
    sub = np.flatnonzero(rng.random(n) < UMI["substituted"])
    umis[sub, rng.integers(0, U, len(sub))] = ACGT[rng.integers(0, 4, len(sub))]
    upk = sa.pack_reads(ReadBatch.fixed(umis), threads=16)
    sample_no = np.ones(n, np.int32)
    ix.set_cell_annotation(feats)
    ix.set_cell_barcodes([r.tobytes() for r in wl])
    c = ix.cell_counter(U, 1)
    c.count_batch(pk, bpk, upk, sample_no)
    c.finish()
    heads, alns, hits, genes, bcno = ix.cell_assign(pk, bpk)
    tc, tf, ts = [], [], []
    for _ in range(reps):
        c.reset()
        t = time.perf_counter()
        c.count_batch(pk, bpk, upk, sample_no)
        tc.append(time.perf_counter() - t)
        t = time.perf_counter()
        got = c.finish()
        tf.append(time.perf_counter() - t)
        t = time.perf_counter()
        ix.cell_assign(pk, bpk)
        ts.append(time.perf_counter() - t)
    ix.set_timing(True)
    ix.cell_align_timing(), ix.cell_assign_timing(), c.timing()
    c.reset()
    c.count_batch(pk, bpk, upk, sample_no)
    c.finish()
    kernels = {k: round(v, 3) for k, v in ix.cell_align_timing().items()}
    kernels.update({"assign_" + k: round(v, 3) for k, v in ix.cell_assign_timing().items()})
    kernels.update({"count_" + k: round(v, 3) for k, v in c.timing().items()})
    ix.set_timing(False)
    c.close()
    ix.close()
    from concurrent.futures import ThreadPoolExecutor
    from tests.cellumi_common import model_lib, model_run
    model_lib()
    cell, gene, u = observations(heads, hits, genes, bcno, umis)
    parts = [np.nonzero((cell % 16 == i) | ((cell < 0) & (i == 0)))[0] for i in range(16)]   # the sections of a cell stay together
    t = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        res = list(ex.map(lambda p: model_run(np.ones(len(p), np.int32), cell[p], gene[p], u[p], U, 1), parts))
    t_model = time.perf_counter() - t
    mc = np.concatenate([r["counts"] for r in res])
    mc = mc[np.lexsort((mc["gene"], mc["cell"]))]
    same = bool(mc.tobytes() == got["counts"].tobytes() and sum(int(r["removed_umis"][0]) for r in res) == int(got["removed_umis"][0]))
    sc, sf, s = float(np.median(tc)), float(np.median(tf)), float(np.median(ts))
    new = sum(v for q, v in kernels.items() if q.startswith("count_"))
    print(json.dumps({"reads": n, "read_length": 100, "total_subreads": 10, "index": "C3 full one-block",
                      "annotation": dict(ANNOT, features=len(feats)), "whitelist": WHITELIST, "umi": UMI, "timed_calls_each": reps,
                      "count_batch_no_result_mreads_per_s": round(n / sc / 1e6, 3), "count_batch_seconds": [round(x, 4) for x in tc],
                      "finish_seconds": [round(x, 4) for x in tf],
                      "cell_assign_mreads_per_s": round(n / s / 1e6, 3), "cell_assign_seconds": [round(x, 4) for x in ts],
                      "host_model_16_threads_seconds": round(t_model, 4),
                      "kernel_ms_one_call": kernels, "new_kernels_share_of_kernel_time": round(new / sum(kernels.values()), 4),
                      "observations": int(len(cell)), "count_table_rows": int(len(got["counts"])), "removed_umis": int(got["removed_umis"][0]),
                      "dropped_no_cell": got["dropped_no_cell"],
                      "bytes_back_per_read": {"count_batch_no_result": 0.0,
                                              "finish_total_bytes": int(got["counts"].nbytes + 40),
                                              "cell_assign": round((heads.nbytes + alns.nbytes + hits.nbytes + genes.nbytes + bcno.nbytes) / n, 1)},
                      "gpu_equals_model": same}), flush=True)


if __name__ == "__main__":
    main()
