// blockplan_check.cc -- svg_blockplan.h against the per-window walk it replaces (host only).
// The walk below is the loop of svg_build.c's build_blocks (build_gene_index,
// index-builder.c:257-357) over a kept bitmap; the planner gets the same bitmap as a prefix array.
// Compared: number of blocks, each block's start, last_set, item count, window range and segments,
// or the 100-block error.  Layouts:
//   * a 17-base contig between larger ones (splits at contig starts), gap 1 and 3
//   * one contig of > 2.1M windows at either gap (deep splits, the 1,999,974 step back)
//   * a single contig under 2 Mbp with a budget far below its items (one block)
//   * a budget reached exactly at a contig's last window
//   * budgets small enough for the 100-block error, at contig starts and deep in a contig
//   * the handle limit (max_blocks)
// over all-kept, seeded random (dense and sparse) and run-structured bitmaps.
// Prints the number of comparisons and exits 0, or the first difference and exits 1.
#include <stdio.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "svg_blockplan.h"

#define PAD 1210
#define MIN_READ_SPLICING 2000000u
#define SPLICE_BACK (MIN_READ_SPLICING - 10 - (MIN_READ_SPLICING - 10) % 3 + 1 - 16)

static long long checks = 0;

struct Layout {
	std::vector<uint32_t> len;
	std::vector<uint64_t> O, wcum;
	int gap;
	uint64_t nwin;
	Layout(const std::vector<uint32_t> &l, int g) : len(l), gap(g)
	{
		uint64_t off = PAD;
		wcum.push_back(0);
		for (uint32_t x : len) {
			O.push_back(off);
			off += (uint64_t)x - 16 + 2 * PAD;
			wcum.push_back(wcum.back() + (x - 16) / gap + 1);
		}
		nwin = wcum.back();
	}
};

struct Seg { uint32_t c; uint64_t a, b; int ends; };
struct Blk { uint64_t start, last_set, items, w_lo, w_hi; std::vector<Seg> segs; };

// the literal walk: false when the 100th block would close
static bool walk(const Layout &L, const std::vector<uint8_t> &kept, uint64_t budget, std::vector<Blk> &out)
{
	out.clear();
	out.push_back(Blk{0, 0, 0, 0, 0, {}});
	for (uint32_t c = 0; c < L.len.size(); c++) {
		const uint64_t last = L.O[c] + (uint64_t)((L.len[c] - 16) / L.gap) * L.gap;
		uint64_t p = L.O[c], a = L.O[c], w = L.wcum[c];   // w: the window at p
		while (p <= last) {
			const uint64_t rl = 16 + p - L.O[c];
			if (kept[w]) out.back().items++;
			if (out.back().items >= budget && (rl > MIN_READ_SPLICING || rl < 32)) {
				out.back().segs.push_back(Seg{c, a, p, 0});
				out.back().last_set = p;
				out.back().w_hi = w;
				if (out.size() == 100) return false;
				p = rl < 32 ? L.O[c] : p - SPLICE_BACK;
				w = L.wcum[c] + (p - L.O[c]) / L.gap;
				out.push_back(Blk{p, 0, 0, w, 0, {}});
				a = p;
				continue;
			}
			p += L.gap;
			w++;
		}
		out.back().segs.push_back(Seg{c, a, last, 1});
		out.back().last_set = L.O[c] + L.len[c] - 16;
		out.back().w_hi = L.wcum[c + 1] - 1;
	}
	return true;
}

// the planner's question answered from a prefix array over the host bitmap
struct Prefix { std::vector<uint64_t> pre; };
static int q_reach(void *ctx, uint64_t w0, uint64_t budget, uint64_t *w)
{
	const Prefix *P = (const Prefix *)ctx;
	if (!budget) { *w = w0; return 1; }
	if (budget > P->pre.back() - P->pre[w0]) return 0;
	// the first w with pre[w + 1] >= pre[w0] + budget
	const uint64_t want = P->pre[w0] + budget;
	*w = (uint64_t)(std::lower_bound(P->pre.begin() + w0 + 1, P->pre.end(), want) - P->pre.begin()) - 1;
	return 1;
}
static int q_count(void *ctx, uint64_t lo, uint64_t hi, uint64_t *n)
{
	const Prefix *P = (const Prefix *)ctx;
	*n = P->pre[hi + 1] - P->pre[lo];
	return 0;
}

#define FAIL(...) do { printf("%s gap %d budget %llu: ", what, L.gap, (unsigned long long)budget); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

static int compare(const char *what, const Layout &L, const std::vector<uint8_t> &kept, uint64_t budget, uint32_t max_blocks,
                   int *nblk_out)
{
	Prefix P;
	P.pre.resize(L.nwin + 1);
	P.pre[0] = 0;
	for (uint64_t w = 0; w < L.nwin; w++) P.pre[w + 1] = P.pre[w] + (kept[w] ? 1 : 0);
	std::vector<Blk> want;
	const bool ok = walk(L, kept, budget, want);
	svg_bp_kept K = {&P, q_reach, q_count};
	svg_blockplan plan;
	const int rc = svg_blockplan_make(L.O.data(), L.len.data(), (uint32_t)L.len.size(), L.gap, budget, max_blocks, &K, &plan);
	checks++;
	if (nblk_out) *nblk_out = ok ? (int)want.size() : -1;
	if (max_blocks && (!ok || want.size() > max_blocks)) {
		const int e = (!ok && max_blocks >= 100) ? SVG_BP_E_WALK : SVG_BP_E_LIMIT;
		if (rc != e) FAIL("planner gave %d, expected error %d (max_blocks %u)", rc, e, max_blocks);
		if (plan.blk || plan.seg) FAIL("a failed plan was not freed");
		return 0;
	}
	if (!ok) {
		if (rc != SVG_BP_E_WALK) FAIL("walk hit the 100-block error, planner gave %d", rc);
		return 0;
	}
	if (rc) FAIL("planner error %d, walk gave %zu blocks", rc, want.size());
	if (plan.nblk != want.size()) FAIL("%u blocks, walk gave %zu", plan.nblk, want.size());
	for (uint32_t k = 0; k < plan.nblk; k++) {
		const svg_bp_block &B = plan.blk[k];
		const Blk &W = want[k];
		checks += 6;
		if (B.start != W.start) FAIL("block %u start %llu != %llu", k, (unsigned long long)B.start, (unsigned long long)W.start);
		if (B.last_set != W.last_set) FAIL("block %u last_set %llu != %llu", k, (unsigned long long)B.last_set, (unsigned long long)W.last_set);
		if (B.items != W.items) FAIL("block %u items %llu != %llu", k, (unsigned long long)B.items, (unsigned long long)W.items);
		if (B.w_lo != W.w_lo || B.w_hi != W.w_hi)
			FAIL("block %u windows [%llu, %llu] != [%llu, %llu]", k, (unsigned long long)B.w_lo, (unsigned long long)B.w_hi,
			     (unsigned long long)W.w_lo, (unsigned long long)W.w_hi);
		if (B.ns != W.segs.size()) FAIL("block %u: %u segments != %zu", k, B.ns, W.segs.size());
		for (uint32_t s = 0; s < B.ns; s++) {
			const svg_bp_seg &S = plan.seg[B.s0 + s];
			const Seg &T = W.segs[s];
			checks += 4;
			if (S.c != T.c || S.a != T.a || S.b != T.b || S.ends != T.ends)
				FAIL("block %u segment %u (%u, %llu, %llu, %d) != (%u, %llu, %llu, %d)", k, s, S.c, (unsigned long long)S.a,
				     (unsigned long long)S.b, S.ends, T.c, (unsigned long long)T.a, (unsigned long long)T.b, T.ends);
		}
	}
	svg_blockplan_free(&plan);
	return 0;
}

static uint64_t rng_state;
static uint32_t rnd(void)
{
	rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)(rng_state >> 33);
}

// kind 0: all kept; 1: 90% kept; 2: 30% kept; 3: runs of 1..400 windows alternately kept and not
// (long stretches without a kept window around the places where blocks close)
static std::vector<uint8_t> bitmap(uint64_t nwin, int kind, uint64_t seed)
{
	std::vector<uint8_t> k(nwin, 1);
	rng_state = seed * 2654435761ull + 12345;
	if (kind == 1 || kind == 2) {
		const uint32_t thr = kind == 1 ? 900 : 300;
		for (uint64_t w = 0; w < nwin; w++) k[w] = rnd() % 1000 < thr;
	} else if (kind == 3) {
		uint8_t v = 0;
		for (uint64_t w = 0; w < nwin;) {
			const uint64_t run = 1 + rnd() % 400;
			for (uint64_t i = 0; i < run && w < nwin; i++) k[w++] = v;
			v = !v;
		}
	}
	return k;
}

int main(void)
{
	const std::vector<uint32_t> synth = {300000, 250000, 17, 200000, 120000};
	const std::vector<uint32_t> deep3 = {6500000, 150000, 900000}, deep1 = {2400000, 150000, 900000};
	const std::vector<uint32_t> lone = {1500000};
	const std::vector<uint32_t> three = {50000, 40000, 30000};
	for (int gap = 1; gap <= 3; gap += 2) {
		int nblk = 0, most = 0;
		// contig starts, a 17-base contig in between
		{
			Layout L(synth, gap);
			for (int kind = 0; kind < 4; kind++) {
				const std::vector<uint8_t> k = bitmap(L.nwin, kind, 100 + kind);
				for (uint64_t budget : {131072ull, 50000ull, 83333ull, 290000ull, 1000ull, 17ull, 100000000ull}) {
					if (compare("synth", L, k, budget, 0, &nblk)) return 1;
					most = std::max(most, nblk);
				}
			}
			if (most < 4) { printf("synth gap %d: no plan of 4 or more blocks (most %d)\n", gap, most); return 1; }
		}
		// deep splits and the step back
		{
			Layout L(gap == 1 ? deep1 : deep3, gap);
			most = 0;
			for (int kind = 0; kind < 4; kind++) {
				const std::vector<uint8_t> k = bitmap(L.nwin, kind, 200 + kind);
				// base: the windows of MIN_READ_SPLICING bases.  A block that starts SPLICE_BACK before the
				// last split moves on only if its budget is reached past the 2M mark again: 1.1 and 1.7
				// base always are, 0.45 base only under the sparse bitmap (the others cycle: 100-block error)
				const uint64_t base = 2000000ull / (unsigned)gap;
				for (uint64_t budget : {base * 11 / 10, base * 17 / 10, base * 45 / 100}) {
					if (budget < base && (kind & 1)) continue;   // (one cycling and one advancing case of these are enough)
					if (compare("deep", L, k, budget, 0, &nblk)) return 1;
					most = std::max(most, nblk);
				}
			}
			{
				// a budget reached long before the 2M mark closes every block at the same window
				const std::vector<uint8_t> k = bitmap(L.nwin, 1, 250);
				if (compare("deep cycle", L, k, 1000, 0, &nblk)) return 1;
				if (nblk != -1) { printf("deep gap %d: budget 1000 did not hit the 100-block error\n", gap); return 1; }
			}
			if (most < 3) { printf("deep gap %d: no plan of 3 or more blocks (most %d)\n", gap, most); return 1; }
			// the handle limit
			const std::vector<uint8_t> k = bitmap(L.nwin, 1, 299);
			for (uint32_t maxb : {1u, 2u, 3u, 64u, 100u, 1000u})
				if (compare("deep limit", L, k, 2200000 / (unsigned)gap, maxb, NULL)) return 1;
			if (compare("deep limit", L, k, 1000, 64, NULL)) return 1;
		}
		// one contig under 2 Mbp: one block whatever the budget
		{
			Layout L(lone, gap);
			for (int kind = 0; kind < 4; kind++) {
				const std::vector<uint8_t> k = bitmap(L.nwin, kind, 300 + kind);
				for (uint64_t budget : {1000ull, 131072ull, 1ull << 40}) {
					if (compare("lone", L, k, budget, 0, &nblk)) return 1;
					if (budget > 16 && nblk != 1) { printf("lone gap %d budget %llu: %d blocks\n", gap, (unsigned long long)budget, nblk); return 1; }
				}
			}
		}
		// a budget reached exactly at a contig's last window (and one window to either side)
		{
			Layout L(three, gap);
			for (int kind = 0; kind < 4; kind++) {
				std::vector<uint8_t> k = bitmap(L.nwin, kind, 400 + kind);
				for (uint32_t c = 0; c < 2; c++) {
					k[L.wcum[c + 1] - 1] = 1;   // the contig's last window is kept: the count lands on it
					uint64_t upto = 0;
					for (uint64_t w = 0; w < L.wcum[c + 1]; w++) upto += k[w];
					for (uint64_t budget : {upto - 1, upto, upto + 1})
						if (compare("last window", L, k, budget, 0, &nblk)) return 1;
				}
			}
		}
		// budgets at or under the 16 bases in which a contig start closes a block: 100-block error
		{
			Layout L(synth, gap);
			const std::vector<uint8_t> k = bitmap(L.nwin, 0, 0);
			for (uint64_t budget : {1ull, 5ull, (unsigned long long)(15 / gap + 1)}) {
				if (compare("start cycle", L, k, budget, 0, &nblk)) return 1;
				if (nblk != -1) { printf("synth gap %d: budget %llu did not hit the 100-block error\n", gap, (unsigned long long)budget); return 1; }
			}
		}
	}
	printf("ok %lld\n", checks);
	return 0;
}
