#!/usr/bin/env python3
"""svg_cell_vote_batch throughput (GPU box): cellCounts' voting step for 100-base simulated reads
on the C3 genome's full one-block index, host buffers in and out (VoteIndex.cell_vote: upload,
probe, tally, compaction, download), beside the same reads through the plain-C model
(tests/native/cellvote_model.c) on 16 threads, whose tables the GPU's are compared with byte for
byte.  Not gated by anything: the reference's own cellCounts loop cannot run where the GPU is.

  bench_cellvote.py [reads (default 4M)] [timed repetitions (default 3)]

One warm-up call, then the median of the timed calls (wall clock around the synchronous entry
point).  The model runs in slices of 256k reads (its staging is 51 records per read).  Prints one
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
from tests.cellvote_common import model_vote, raw  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4 << 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    g = random_genome(c3_lengths(), 3000, repeats=(1_000_000, 300, 200, 0.12))
    reads = simulate_reads(g, n, 100, threads=16)
    pk = sa.pack_reads(reads, threads=16)
    ix = sa.VoteIndex.build_genome(g, gap=1, memory_mb=8000, force_one_block=True, device=0)
    heads, slots = ix.cell_vote(pk)
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        ix.cell_vote(pk)
        times.append(time.perf_counter() - t)
    index = ix.export()
    ix.close()
    tm, same, at = 0.0, True, 0
    for o in range(0, n, 1 << 18):
        part = reads.slice(o, min(n, o + (1 << 18)))
        t = time.perf_counter()
        mh, ms = model_vote(index, part, 10, threads=16)
        tm += time.perf_counter() - t
        k = len(part)
        # (first_slot counts from the slice's start in the model's heads; a skipped read's is 0)
        voted = mh["applied_subreads"] > 0
        same &= bool((heads[o:o + k]["first_slot"][voted] == mh["first_slot"][voted] + at).all())
        same &= all(np.array_equal(mh[f], heads[o:o + k][f]) for f in ("n_slots", "max_vote", "applied_subreads", "items"))
        same &= bool((raw(ms) == raw(slots[at:at + len(ms)])).all())
        at += len(ms)
    same &= at == len(slots)
    tg = float(np.median(times))
    print(json.dumps({"reads": n, "read_length": 100, "total_subreads": 10, "index": "C3 full one-block",
                      "gpu_mreads_per_s": round(n / tg / 1e6, 3), "gpu_seconds": [round(x, 4) for x in times],
                      "model16_mreads_per_s": round(n / tm / 1e6, 3), "model_threads": 16,
                      "slots_per_read": round(len(slots) / n, 2), "voted_fraction": round(float((heads["max_vote"] > 0).mean()), 4),
                      "gpu_equals_model": same}), flush=True)


if __name__ == "__main__":
    main()
