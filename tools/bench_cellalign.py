#!/usr/bin/env python3
"""svg_cell_align_batch throughput (GPU box), beside svg_cell_vote_batch on the same reads in the
same process: 100-base simulated reads on the C3 genome's full one-block index, 10 subreads, host
buffers in and out (VoteIndex.cell_align / VoteIndex.cell_vote).  For the record only: nothing is
gated by it.

  bench_cellalign.py [reads (default 4,194,304)] [timed repetitions (default 3)]

One warm-up call of each, then the median of the timed calls (wall clock around the synchronous
entry points), alternating the two.  Then one more cell_align call under svg_set_timing for the
per-kernel milliseconds (HIP events around each launch, summed over the chunks).  The first 65,536
reads' answers are compared with the plain-C model (tests/native/cellalign_model.c).  Prints one
JSON object."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import subread_amd as sa  # noqa: E402
from subread_amd.sim import random_genome, c3_lengths, simulate_reads  # noqa: E402
from tests.cellalign_common import model_align, raw  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4 << 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    g = random_genome(c3_lengths(), 3000, repeats=(1_000_000, 300, 200, 0.12))
    reads = simulate_reads(g, n, 100, threads=16)
    pk = sa.pack_reads(reads, threads=16)
    ix = sa.VoteIndex.build_genome(g, gap=1, memory_mb=8000, force_one_block=True, device=0)
    heads, alns = ix.cell_align(pk)
    vh, vs = ix.cell_vote(pk)
    ta, tv = [], []
    for _ in range(reps):
        t = time.perf_counter()
        ix.cell_align(pk)
        ta.append(time.perf_counter() - t)
        t = time.perf_counter()
        ix.cell_vote(pk)
        tv.append(time.perf_counter() - t)
    ix.set_timing(True)
    ix.cell_align_timing()
    ix.cell_align(pk)
    kernels = {k: round(v, 3) for k, v in ix.cell_align_timing().items()}
    ix.set_timing(False)
    # (a one-block index built from a genome: its .array image starts at base 0)
    index = ix.export()
    index = dict(index, values=np.ascontiguousarray(index["values"][:index["values_bytes"]]), start_base_offset=0)
    m = min(n, 1 << 16)
    mh, ma = model_align(index, reads.slice(0, m))
    k = int(heads["n_records"][:m].sum())
    same = bool((raw(mh) == raw(heads[:m])).all() and len(ma) == k and (raw(ma) == raw(alns[:k])).all())
    ix.close()
    a, v = float(np.median(ta)), float(np.median(tv))
    print(json.dumps({"reads": n, "read_length": 100, "total_subreads": 10, "index": "C3 full one-block",
                      "cell_align_mreads_per_s": round(n / a / 1e6, 3), "cell_align_seconds": [round(x, 4) for x in ta],
                      "cell_vote_mreads_per_s": round(n / v / 1e6, 3), "cell_vote_seconds": [round(x, 4) for x in tv],
                      "cell_align_kernel_ms": kernels, "records_per_read": round(len(alns) / n, 4),
                      "bytes_back_per_read": {"cell_align": round((heads.nbytes + alns.nbytes) / n, 1),
                                              "cell_vote": round((vh.nbytes + vs.nbytes) / n, 1)},
                      "gpu_equals_model_first_65536": same}), flush=True)


if __name__ == "__main__":
    main()
