#!/usr/bin/env python3
"""CPU model of the lane kernel's lockstep cost under a count-bin rule (svg_lane.hip,
lane_bin_kernel / lane_kernel).  A lane owns a read; a wave runs, for strand 0 and then for strand
1, as many vote-loop steps as its heaviest lane has candidates on that strand.  Given per-read
(strand-0, strand-1) candidate counts the model forms the 64-read groups a rule would form and
sums max(c0) + max(c1) over them: the quantity the device adds to word 28 of svg_debug_counters
with statistics on.  Lane utilisation = candidates / (64 * steps).

Rules (steps(counts, rule, ...)):
  "none"   groups of 64 consecutive reads
  "max"    four lists by the larger strand count (<= 8, <= 16, <= 24, <= 40), each in tile order
  "strand" eight lists, heavier strand x class of its count; with light_edges, a tile's part of a
           list is ordered by the class of the lighter strand's count (the kernel's LLIGHT > 1;
           the shipped kernel keeps read order, light_edges=())
Reads with more than `cap` candidates on a strand are deferred and take no lane.  The device
appends tiles to a list in the order their blocks arrive; the model appends them in read order.

Usage: lane_bin_model.py [--counts FILE.npy | --reads N] [--tile T] [--json OUT]
Without --counts a C3-like sample is drawn (c3_like_counts): per strand Poisson chance hits of 10
probes in a 3 Gbp full index, plus the read's true hits on its own strand, plus a share of reads
from repeat families."""
import argparse
import json
import sys

import numpy as np

HEAVY_EDGES = (8, 16, 24)          # lbin_of: <= 8, <= 16, <= 24, the rest
# llight_of: 0..11 each their own class, then 12-15, 16-19, 20-23, >= 24
LIGHT_EDGES = tuple(range(0, 12)) + (15, 19, 23)
CAP = 40


def classes(c, edges):
    """class of each count: the number of edges below it (count <= edges[k] -> class <= k)"""
    return np.searchsorted(np.asarray(edges), c, side="left")


def group_steps(c0, c1, order):
    """sum over 64-read groups of `order` (read numbers, list order) of max c0 + max c1"""
    if len(order) == 0:
        return 0, 0
    pad = (-len(order)) % 64
    a = np.concatenate([c0[order], np.zeros(pad, c0.dtype)]).reshape(-1, 64)
    b = np.concatenate([c1[order], np.zeros(pad, c1.dtype)]).reshape(-1, 64)
    return int(a.max(1).sum() + b.max(1).sum()), a.shape[0]


def lists_of(c0, c1, rule, tile=1024, light_edges=(), cap=CAP):
    """the rule's lists, heaviest first: arrays of read numbers in list order"""
    n = len(c0)
    r = np.arange(n)
    mx, mn = np.maximum(c0, c1), np.minimum(c0, c1)
    keep = mx <= cap
    if rule == "none":
        return [r[keep]]
    h = classes(mx, HEAVY_EDGES)
    if rule == "max":
        return [r[keep & (h == k)] for k in range(len(HEAVY_EDGES), -1, -1)]
    if rule != "strand":
        raise ValueError(rule)
    hv = (c1 > c0).astype(np.int64)              # the heavier strand (ties: strand 0)
    lc = classes(mn, light_edges)
    out = []
    for k in range(len(HEAVY_EDGES), -1, -1):
        for o in (1, 0):
            sel = r[keep & (h == k) & (hv == o)]
            # tile order, inside a tile by light class, inside a class by read number
            out.append(sel[np.lexsort((sel, lc[sel], sel // tile))])
    return out


def steps(c0, c1, rule, tile=1024, light_edges=(), cap=CAP, chunk=0):
    """(vote-loop steps, groups, candidates on lanes) of a rule; lists are made per chunk of reads"""
    c0, c1 = np.asarray(c0, np.int64), np.asarray(c1, np.int64)
    n = len(c0)
    chunk = chunk or max(n, 1)
    s = g = 0
    for a in range(0, n, chunk):
        x, y = c0[a:a + chunk], c1[a:a + chunk]
        for lst in lists_of(x, y, rule, tile, light_edges, cap):
            ds, dg = group_steps(x, y, lst)
            s, g = s + ds, g + dg
    keep = np.maximum(c0, c1) <= cap
    return s, g, int((c0 + c1)[keep].sum())


def c3_like_counts(n, seed=1, genome=3.0e9, probes=10, sub=0.01, repeat_share=0.12, repeat_hits=110):
    """per-read counts like C3's: 100-bp reads, 10 probes per strand on a full 3 Gbp index.  A
    probe's 16-mer has genome / 4^16 chance hits; the read's own strand adds one true hit per probe
    whose 16 bases carry no substitution; a share of the reads comes from repeat families whose
    members all hit (those pass the cap and are deferred)."""
    rng = np.random.default_rng(seed)
    lam = probes * genome / 4.0 ** 16
    c = rng.poisson(lam, (n, 2))
    own = rng.integers(0, 2, n)
    true_hits = rng.binomial(probes, (1.0 - sub) ** 16, n)
    rep = rng.random(n) < repeat_share
    true_hits = np.where(rep, rng.poisson(repeat_hits, n), true_hits)
    c[np.arange(n), own] += true_hits
    return c[:, 0], c[:, 1]


def report(c0, c1, tile, chunk):
    rows = {}
    for name, rule, kw in (("consecutive reads", "none", {}), ("max (lane_bins 1)", "max", {}),
                           ("strand, light unordered (lane_bins 0)", "strand", {}),
                           ("strand, light <=4,8,12,16,24", "strand", {"light_edges": (4, 8, 12, 16, 24)}),
                           ("strand, light llight_of (LLIGHT 16)", "strand", {"light_edges": LIGHT_EDGES}),
                           ("strand, light exact", "strand", {"light_edges": tuple(range(CAP))})):
        s, g, cand = steps(c0, c1, rule, tile=tile, chunk=chunk, **kw)
        rows[name] = {"steps": s, "groups": g, "candidates": cand, "steps_per_group": round(s / max(g, 1), 2),
                      "utilisation": round(cand / (64.0 * max(s, 1)), 4)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="", help=".npy of shape (n, 2): strand-0 and strand-1 candidate counts per read")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--tile", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=1_000_000)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if a.counts:
        c = np.load(a.counts)
        c0, c1 = c[:, 0], c[:, 1]
    else:
        c0, c1 = c3_like_counts(a.reads)
    out = {"reads": int(len(c0)), "tile": a.tile, "chunk": a.chunk, "sample": a.counts or "c3_like_counts",
           "mean_candidates": round(float((c0 + c1).mean()), 2)}
    for t in sorted({1024, 4096, a.tile}):
        out["tile_%d" % t] = report(c0, c1, t, a.chunk)
    for t in sorted({1024, 4096, a.tile}):
        print("tile %d" % t)
        for k, v in out["tile_%d" % t].items():
            print("  %-40s steps %11d  groups %7d  steps/group %6.2f  utilisation %.3f" % (
                k, v["steps"], v["groups"], v["steps_per_group"], v["utilisation"]))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
