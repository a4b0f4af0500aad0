#!/usr/bin/env python3
"""Generates tests/golden/fragile/fragile.npz with the REFERENCE's own fragile junction voting
(core_fragile_junction_voting, core-junction.c:5151-5422): oracle/_ref/subjunc-dump run with -T 1
and SVG_REF_FRAGILE, which makes oracle/ref_dump_hook.c dump every window's finished vote table
(as select_best_vote receives it), its start and length, and the junction the window supported.
Runs only in the survey container (it needs /root/reference for the oracle/_ref build).

Genome fredge (tests/common.py); indexes fredge_full and fredge_gapped built by the reference's
subread-buildindex, their md5 known answers (and fredge_fullM1's) added to
tests/golden/index_md5.json.  Read sets per index: `se` -- one read of every class of
tests.common.fredge_reads at every length of FREDGE_LENGTHS; `pe` -- pairs at the lengths PE_LENGTHS
(tests/fragile_common.py),
the two ends of a pair differing in length (161 with 181, 181 with 241, 241 with 700, 700 with 161).

The golden holds data only: the reads, their class tags and strands, and the dump, column by column
(tests/fragile_common.py reads it back)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
from tests.common import GOLD, IndexCache, fredge_reads  # noqa: E402
from tests.fragile_common import REF_WIN_DTYPE, REF_SLOT_DTYPE, GOLDEN_SETS, AMBIGUOUS_CAP, PE_LENGTHS  # noqa: E402
from tests.golden.make_golden import build_ref_index  # noqa: E402
from subread_amd.sim import write_fastq  # noqa: E402

REFBIN = os.path.join(ROOT, "oracle", "_ref")
MD5_KEYS = ["fredge_full", "fredge_gapped", "fredge_fullM1"]
SEEDS = {"se": 31, "pe": 47}


def read_set(kind):
    if kind == "se":
        return fredge_reads(1, SEEDS[kind])
    return fredge_reads(1, SEEDS[kind], lengths=PE_LENGTHS, paired=True)


def run_ref(pre, reads, d):
    f1, f2 = os.path.join(d, "r1.fq"), None
    write_fastq(f1, reads.r1)
    dump = os.path.join(d, "fragile.bin")
    if os.path.exists(dump):
        os.remove(dump)
    args = [REFBIN + "/subjunc-dump", "-T", "1", "-i", pre, "-r", f1, "-o", os.path.join(d, "out.sam")]
    if reads.r2 is not None:
        f2 = os.path.join(d, "r2.fq")
        write_fastq(f2, reads.r2)
        args += ["-R", f2]
    r = subprocess.run(args, env=dict(os.environ, SVG_REF_FRAGILE=dump), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
    b = open(dump, "rb").read()
    wins, slots, o = [], [], 0
    while o < len(b):
        w = np.frombuffer(b, REF_WIN_DTYPE, 1, o)
        o += REF_WIN_DTYPE.itemsize
        n = int(w["n_used"][0])
        wins.append(w)
        slots.append(np.frombuffer(b, REF_SLOT_DTYPE, n, o))
        o += REF_SLOT_DTYPE.itemsize * n
    assert o == len(b)
    return np.concatenate(wins), np.concatenate(slots)


def main():
    assert os.path.exists(REFBIN + "/subjunc-dump"), "build oracle/_ref first (make -C oracle)"
    out, note = {}, {}
    with tempfile.TemporaryDirectory() as d:
        cache = IndexCache(d)
        mpath = os.path.join(GOLD, "index_md5.json")
        meta = json.load(open(mpath))
        for key in MD5_KEYS:
            if key not in meta["md5"]:
                meta["md5"][key] = build_ref_index(cache.genome_fasta("fredge"), os.path.join(d, "ref_" + key), key)
        with open(mpath, "w") as f:
            json.dump(meta, f, indent=1)
        for name in GOLDEN_SETS:
            key, kind = name.rsplit("_", 1)
            pre = cache.get(key)   # our builder's index, md5-checked against the reference's
            reads = read_set(kind)
            w, s = run_ref(pre, reads, d)
            junction = w["junction"] == 1
            amb = junction & (w["large_side"] == 0xffffffff)
            share = float(amb.sum()) / max(1, int(junction.sum()))
            note[name] = dict(reads=len(reads.r1), windows=len(w), slots=len(s), junction_windows=int(junction.sum()),
                              ambiguous_large_side=int(amb.sum()), ambiguous_share=round(share, 5))
            print(name, note[name])
            if share > AMBIGUOUS_CAP:
                raise SystemExit("%s: %.2f%% of the junction windows have an ambiguous large side (cap %.0f%%)"
                                 % (name, 100 * share, 100 * AMBIGUOUS_CAP))
            for e, rb in (("r1", reads.r1), ("r2", reads.r2)):
                if rb is not None:
                    out["%s.%s_seq" % (name, e)], out["%s.%s_off" % (name, e)], out["%s.%s_len" % (name, e)] = rb.seq, rb.offsets, rb.lens
            out[name + ".cls"], out[name + ".strand"] = reads.cls.astype("S"), reads.strand
            for fld in REF_WIN_DTYPE.names:
                out["%s.w.%s" % (name, fld)] = np.ascontiguousarray(w[fld])
            for fld in REF_SLOT_DTYPE.names:
                out["%s.s.%s" % (name, fld)] = np.ascontiguousarray(s[fld].T)
    out["note"] = np.array(json.dumps(note))
    path = os.path.join(HERE, "fragile.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
