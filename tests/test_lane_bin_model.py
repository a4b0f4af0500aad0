"""CPU: tools/lane_bin_model.py against the definition of the device's step counter (word 28 of
svg_debug_counters: per 64-read group and strand, the largest candidate count of a lane), on
hand-made counts and against a read-by-read restatement of lane_bin_kernel's keys."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import lane_bin_model as m  # noqa: E402


def test_classes_are_the_kernels():
    """lbin_of and llight_of of svg_lane.hip"""
    lbin = [0 if c <= 8 else 1 if c <= 16 else 2 if c <= 24 else 3 for c in range(41)]
    light = [c if c < 12 else 12 + ((c - 12) >> 2) if c < 24 else 15 for c in range(41)]
    assert list(m.classes(np.arange(41), m.HEAVY_EDGES)) == lbin
    assert list(m.classes(np.arange(41), m.LIGHT_EDGES)) == light


def test_hand_made_counts():
    # 64 reads heavy on strand 0 interleaved with 64 heavy on strand 1: one list by the larger
    # count alone gives two groups of (10, 10); by strand two groups of (10, 2) and (2, 10)
    c0 = np.array([10, 2] * 64)
    c1 = np.array([2, 10] * 64)
    assert m.steps(c0, c1, "none")[:2] == (40, 2)
    assert m.steps(c0, c1, "max")[:2] == (40, 2)
    assert m.steps(c0, c1, "strand") == (24, 2, 128 * 12)
    # 128 reads of (12, 1) and (12, 7) alternating: unordered, both groups run 12 + 7; ordered by
    # the light strand inside one 128-read tile, 12 + 1 and 12 + 7; 64-read tiles order nothing
    # across the two groups
    c0 = np.full(128, 12)
    c1 = np.array([1, 7] * 64)
    assert m.steps(c0, c1, "strand", tile=128, light_edges=())[0] == 38
    assert m.steps(c0, c1, "strand", tile=128, light_edges=m.LIGHT_EDGES)[0] == 13 + 19
    assert m.steps(c0, c1, "strand", tile=64, light_edges=m.LIGHT_EDGES)[0] == 38
    # a read past the cap takes no lane; one more light read opens a list and a group of its own
    c0 = np.concatenate([c0, [41, 3]])
    c1 = np.concatenate([c1, [0, 0]])
    assert m.steps(c0, c1, "strand", tile=128, light_edges=m.LIGHT_EDGES) == (13 + 19 + 3, 3, 128 * 12 + 64 * 8 + 3)
    # lists are made per chunk: two chunks of 65 reads make two partly filled groups each
    c0 = np.full(130, 5)
    c1 = np.zeros(130, int)
    assert m.steps(c0, c1, "strand", chunk=65)[:2] == (20, 4)
    assert m.steps(c0, c1, "strand")[:2] == (15, 3)


def device_steps(c0, c1, rule, tile, llight=16):
    """lane_bin_kernel and lane_kernel restated read by read: key = (list, light class), tiles
    appended in order, groups of 64 from list 7 down"""
    lists = [[] for _ in range(8)]
    for t0 in range(0, len(c0), tile):
        keyed = []
        for r in range(t0, min(t0 + tile, len(c0))):
            mx, mn = max(c0[r], c1[r]), min(c0[r], c1[r])
            if mx > 40:
                continue
            h = 0 if mx <= 8 else 1 if mx <= 16 else 2 if mx <= 24 else 3
            lc = 0 if llight == 1 else mn if mn < 12 else 12 + ((mn - 12) >> 2) if mn < 24 else 15
            keyed.append((2 * h, 0, r) if rule == 1 else (2 * h + (1 if c1[r] > c0[r] else 0), lc, r))
        for l, _, r in sorted(keyed):
            lists[l].append(r)
    s = 0
    for l in range(7, -1, -1):
        for a in range(0, len(lists[l]), 64):
            g = lists[l][a:a + 64]
            s += max(c0[r] for r in g) + max(c1[r] for r in g)
    return s


def test_model_is_the_device_definition():
    rng = np.random.default_rng(7)
    c0, c1 = m.c3_like_counts(5000, seed=3)
    c0[:40] = rng.integers(0, 45, 40)      # ties, zeros, counts at and past the cap
    c1[:40] = c0[:40][::-1]
    c0[40:60] = c1[40:60]
    for tile in (256, 1024, 4096):
        assert m.steps(c0, c1, "strand", tile=tile)[0] == device_steps(c0, c1, 0, tile, 1)
        assert m.steps(c0, c1, "strand", tile=tile, light_edges=m.LIGHT_EDGES)[0] == device_steps(c0, c1, 0, tile, 16)
        assert m.steps(c0, c1, "max", tile=tile)[0] == device_steps(c0, c1, 1, tile)
    assert m.steps(c0, c1, "strand")[0] < m.steps(c0, c1, "max")[0]
