/* svg_blockplan.h -- where a multi-block index splits (build_gene_index, index-builder.c:257-357),
 * planned from the contig layout and ONE question about the repeat scan's result, without a walk
 * over every window.  Plain C, no dependency beyond libc: the GPU builder (svg_gpubuild.hip)
 * answers the question from its kept bitmap in HBM, tests/native/blockplan_check.cc from a host
 * bitmap.
 *
 * Windows are numbered in genome order: window w = wcum[c] + t is the t-th sampled 16-mer of contig
 * c, at linear position O[c] + t * gap.  A window is "kept" when its key is no repeat.
 *
 *   - A block counts its kept windows; it can close only once that count has reached `budget`.
 *   - It then closes at the first window at or after that point, kept or not, whose
 *     rl = 16 + p - O[c] is < 32 or > MIN_READ_SPLICING.  That window still belongs to the block.
 *   - The next block starts at O[c] when rl < 32, else SPLICE_BACK bases before p (a multiple of 3:
 *     gap-3 windows stay on their lattice), and counts again from there: blocks overlap, and each
 *     is one contiguous range [w_lo, w_hi] of window numbers.
 *
 * After the answer to "which window reaches the budget" everything is arithmetic: the windows with
 * rl < 32 are the first ones of a contig (t * gap < 16), those with rl > MIN_READ_SPLICING start
 * at t = (MIN_READ_SPLICING - 16) / gap + 1.
 */
#ifndef SVG_BLOCKPLAN_H
#define SVG_BLOCKPLAN_H
#include <stdint.h>
#include <stdlib.h>

#define SVG_BP_MIN_READ_SPLICING 2000000u
#define SVG_BP_SPLICE_BACK (SVG_BP_MIN_READ_SPLICING - 10 - (SVG_BP_MIN_READ_SPLICING - 10) % 3 + 1 - 16)   /* 1,999,974 */
#define SVG_BP_WALK_BLOCKS 100   /* the reference's two-digit block number */

/* results other than 0; a negative value is a callback's own error, passed through */
#define SVG_BP_E_WALK   1   /* a 101st block would be needed */
#define SVG_BP_E_LIMIT  2   /* more than max_blocks blocks */
#define SVG_BP_E_NOMEM  3

/* windows [a, b] (linear positions, step gap) of contig c; ends: the segment runs to the contig's
 * last window, and the block then holds the contig's bases to its very end */
typedef struct svg_bp_seg { uint32_t c; uint64_t a, b; int ends; } svg_bp_seg;
/* start: position of the block's first window (0 for the first block); last_set: position of the
 * last window written (or contig end - 16); segments seg[s0 .. s0 + ns) */
typedef struct svg_bp_block { uint64_t start, last_set, items, w_lo, w_hi; uint32_t s0, ns; } svg_bp_block;
typedef struct svg_blockplan { svg_bp_block *blk; svg_bp_seg *seg; uint32_t nblk, nseg, blkcap, segcap; } svg_blockplan;

typedef struct svg_bp_kept {
	void *ctx;
	/* THE question: the first window w >= w0 such that [w0, w] holds `budget` kept windows.
	 * 1 and *w, 0 when there is none, < 0 on an error */
	int (*reach)(void *ctx, uint64_t w0, uint64_t budget, uint64_t *w);
	/* kept windows in [w_lo, w_hi]: only reported (svg_bp_block.items), never decided upon; 0, or < 0 on
	 * an error */
	int (*count)(void *ctx, uint64_t w_lo, uint64_t w_hi, uint64_t *n);
} svg_bp_kept;

static inline void svg_blockplan_free(svg_blockplan *P)
{
	free(P->blk); free(P->seg);
	P->blk = NULL; P->seg = NULL;
	P->nblk = P->nseg = P->blkcap = P->segcap = 0;
}

static inline int svg_bp_push_seg(svg_blockplan *P, uint32_t c, uint64_t a, uint64_t b, int ends)
{
	if (P->nseg == P->segcap) {
		uint32_t cap = P->segcap ? 2 * P->segcap : 64;
		svg_bp_seg *s = (svg_bp_seg *)realloc(P->seg, sizeof(svg_bp_seg) * cap);
		if (!s) return SVG_BP_E_NOMEM;
		P->seg = s; P->segcap = cap;
	}
	P->seg[P->nseg].c = c; P->seg[P->nseg].a = a; P->seg[P->nseg].b = b; P->seg[P->nseg].ends = ends;
	P->nseg++;
	P->blk[P->nblk - 1].ns++;
	return 0;
}

static inline int svg_bp_new_block(svg_blockplan *P, uint64_t start, uint64_t w_lo)
{
	svg_bp_block *B;
	if (P->nblk == P->blkcap) {
		uint32_t cap = P->blkcap ? 2 * P->blkcap : 16;
		svg_bp_block *b = (svg_bp_block *)realloc(P->blk, sizeof(svg_bp_block) * cap);
		if (!b) return SVG_BP_E_NOMEM;
		P->blk = b; P->blkcap = cap;
	}
	B = &P->blk[P->nblk++];
	B->start = start; B->last_set = 0; B->items = 0; B->w_lo = w_lo; B->w_hi = w_lo; B->s0 = P->nseg; B->ns = 0;
	return 0;
}

/* position of contig c's last window */
static inline uint64_t svg_bp_last_window(const uint64_t *O, const uint32_t *len, uint32_t c, int gap)
{
	return O[c] + (uint64_t)((len[c] - 16) / (uint32_t)gap) * (uint64_t)gap;
}

/*
 * The blocks of an index over contigs of len[c] > 16 bases at linear positions O[c], windows every
 * `gap` bases, `budget` items per block.  max_blocks > 0: SVG_BP_E_LIMIT instead of a block beyond
 * that many (what a handle can hold).  *P is filled (svg_blockplan_free it) when 0 comes back and
 * freed otherwise.  A plan of one block is the ordinary case of a genome of short contigs.
 */
static inline int svg_blockplan_make(const uint64_t *O, const uint32_t *len, uint32_t nctg, int gap, uint64_t budget,
                                     uint32_t max_blocks, const svg_bp_kept *K, svg_blockplan *P)
{
	uint64_t *wcum = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)nctg + 1));
	uint64_t w0 = 0, start = 0, a, nwin;
	uint32_t c0 = 0, c;
	int rc = 0;
	P->blk = NULL; P->seg = NULL;
	P->nblk = P->nseg = P->blkcap = P->segcap = 0;
	if (!wcum) return SVG_BP_E_NOMEM;
	wcum[0] = 0;
	for (c = 0; c < nctg; c++) wcum[c + 1] = wcum[c] + (len[c] - 16) / (uint32_t)gap + 1;
	nwin = wcum[nctg];
	a = O[0];
	for (;;) {
		svg_bp_block *B;
		uint64_t wq = 0, wc = 0;
		int closes;
		if ((rc = svg_bp_new_block(P, start, w0))) break;
		closes = K->reach(K->ctx, w0, budget, &wq);
		if (closes < 0) { rc = closes; break; }
		if (closes) {
			/* the first window at or after wq with rl < 32 or rl > MIN_READ_SPLICING */
			uint64_t t, d;
			c = c0;
			while (wcum[c + 1] <= wq) c++;
			t = wq - wcum[c];
			d = t * (uint64_t)gap;   /* p - O[c] */
			if (d < 16 || d + 16 > SVG_BP_MIN_READ_SPLICING) wc = wq;
			else {
				const uint64_t t2 = (SVG_BP_MIN_READ_SPLICING - 16) / (uint32_t)gap + 1;
				if (t2 < wcum[c + 1] - wcum[c]) wc = wcum[c] + t2;
				else if (c + 1 < nctg) wc = wcum[c + 1];   /* the next contig's first window: rl = 16 */
				else closes = 0;
			}
		}
		if (!closes) {
			/* runs to the genome's end */
			for (c = c0; c < nctg && !rc; c++)
				rc = svg_bp_push_seg(P, c, c == c0 ? a : O[c], svg_bp_last_window(O, len, c, gap), 1);
			if (rc) break;
			B = &P->blk[P->nblk - 1];
			B->last_set = O[nctg - 1] + len[nctg - 1] - 16;
			B->w_hi = nwin - 1;
			rc = K->count(K->ctx, B->w_lo, B->w_hi, &B->items);
			break;
		}
		{
			uint32_t cc = c0;
			uint64_t p, rl;
			while (wcum[cc + 1] <= wc) cc++;
			p = O[cc] + (wc - wcum[cc]) * (uint64_t)gap;
			for (c = c0; c < cc && !rc; c++)
				rc = svg_bp_push_seg(P, c, c == c0 ? a : O[c], svg_bp_last_window(O, len, c, gap), 1);
			if (!rc) rc = svg_bp_push_seg(P, cc, cc == c0 ? a : O[cc], p, 0);
			if (rc) break;
			B = &P->blk[P->nblk - 1];
			B->last_set = p;
			B->w_hi = wc;
			rc = K->count(K->ctx, B->w_lo, B->w_hi, &B->items);
			if (rc) break;
			if (P->nblk == SVG_BP_WALK_BLOCKS) { rc = SVG_BP_E_WALK; break; }
			if (max_blocks && P->nblk == max_blocks) { rc = SVG_BP_E_LIMIT; break; }
			rl = 16 + p - O[cc];
			if (rl < 32) { start = O[cc]; w0 = wcum[cc]; }
			else { start = p - SVG_BP_SPLICE_BACK; w0 = wc - SVG_BP_SPLICE_BACK / (uint32_t)gap; }
			a = start;
			c0 = cc;
		}
	}
	free(wcum);
	if (rc) svg_blockplan_free(P);
	return rc;
}

#endif
