// svg_cell_align.hip -- cellCounts' step behind the vote for a batch of reads (include/subread_vote.h
// svg_cell_align_batch): cellCounts_select_and_write_alignments (cell-counts.c:2648-2719) up to its
// calls of the writer, on the vote tables that svg_cell.hip's probe and tally kernels leave in HBM.
//
// Per chunk of reads, after cell_probe_kernel and cell_tally_kernel (cell_launch_vote):
//   align_select_kernel   lane = read: the at most max_voting_simples table slots in the reference's
//       visiting order (:2654-2686), one byte each, slot-major.
//   align_explain_kernel  lane = (read, candidate): cellCounts_explain_one_read (:2520-2627).  All
//       base work goes through mismatch masks in LDS: the strand's 160 read codes (the reference's
//       read_bin, 2 bits a base, LSB first) against the .array image at abs_pos + section offset,
//       one bit per base at bit 2 * (i & 15) of word i >> 4.  Two masks are live: the current
//       section's offset and the next one's.  matchBin_chro is a popcount over a range, the
//       soft-clip scans and the meet in the middle walk bits.  The CIGAR goes through
//       reduce_Cigar's merge piece by piece ('-' of a negative number is an operation of count 1
//       to it) straight into the candidate's record; the exon weight is taken at each flush.
//   align_emit_kernel     lane = read: quick_sort's order of the scores (core.c:4690-4714, on an
//       explicit stack as in cell_tally_kernel) and the records to write (:2700-2716).
//   align_scan_kernel, align_compact_kernel  exclusive sum of the record counts (one block), then
//       the chosen candidate records copied to their place.
// svg_cell_set_exons: align_exon_kernel, thread = interval, ORs the two bit planes (:938-959).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "subread_vote.h"
#include "svg_internal.h"
#include "svg_device.h"
#include "svg_keylookup.h"
#include "svg_cell.h"

#define A_WORDS   10                   // 160 bases, 16 to a word
#define A_IND     21                   // MAX_INDEL_TOLERANCE * 3
#define A_INVALID (-9999999)           // MINM_INVALID_INDEL
#define A_TOP     10000000ll           // SCORING_MAX_QUALITY_MAPPING
#define A_STACK   8

struct AlignParams {
	CellParams cp;
	svg_cell_align_params p;
	int max_simples;
	const uint8_t *values;
	uint32_t values_bytes, sbo;
	const uint32_t *planes;            // two planes of plane_bits bits, or NULL
	uint64_t plane_bits;
	uint8_t *cand;                     // [max_simples][n]: table slot of candidate c
	uint8_t *ncand;                    // [n]
	svg_cell_aln *crec;                // [n][max_simples]
	uint8_t *order;                    // [max_simples][n]: candidate of the read's k-th record
	svg_cell_aln_head *aheads;         // [n]
	svg_cell_aln *compact;
	uint64_t rec_base;
	uint64_t *total;
	uint32_t *overflow;               // candidates whose CIGAR text did not fit its field
};

__global__ void __launch_bounds__(256) align_select_kernel(AlignParams ap)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r >= ap.cp.n) return;
	const svg_cell_head *h = ap.cp.heads + r;
	const svg_cell_slot *stage = ap.cp.staging + (size_t)r * C_SLOTS;
	int count = 0;
	// (one subread per strand: find_subread_end divides by zero in the reference; no candidates)
	if (h->applied_subreads >= 2 && h->max_vote >= ap.p.min_votes_per_mapped_read) {
		int t0 = 0, t1 = 0, t2 = 0;    // cellCounts_update_top_three (:2296-2310)
		for (int row = 0; row < SVG_CELL_ROWS; row++)
			for (int it = 0; it < h->items[row]; it++) {
				const int v = stage[row * SVG_CELL_SPACE + it].votes;
				if (v < ap.p.min_votes_per_mapped_read || v <= t2) continue;
				if (v > t0) { t2 = t1; t1 = t0; t0 = v; }
				else if (v == t0) ;
				else if (v > t1) { t2 = t1; t1 = v; }
				else if (v == t1) ;
				else t2 = v;
			}
		for (int d = 0; d < 3 && count < ap.max_simples; d++) {
			const int N = d == 0 ? t0 : d == 1 ? t1 : t2;
			if (N < 1 || t0 - N > ap.p.max_differential_from_top_vote_number) break;
			for (int row = 0; row < SVG_CELL_ROWS && count < ap.max_simples; row++)
				for (int it = 0; it < h->items[row] && count < ap.max_simples; it++)
					if (stage[row * SVG_CELL_SPACE + it].votes == N)
						ap.cand[(size_t)count++ * ap.cp.n + r] = (uint8_t)(row * SVG_CELL_SPACE + it);
		}
	}
	ap.ncand[r] = (uint8_t)count;
}

// ---------------------------------------------------------------------------------------------
// the explain kernel's per-lane LDS
struct AlignLds {
	uint32_t rd[A_WORDS][64];          // the strand's read codes, LSB first
	uint32_t tmp[A_WORDS][64];
	uint32_t mk[2][A_WORDS][64];       // mismatch masks
	int16_t ind[A_IND][64];            // indel_offsets
	int8_t off[C_SUB][64];             // indel_recorder_copy's offsets
};

// the code of the genome base at linear position pos; outside the image: 0 (subread_vote.h)
__device__ __forceinline__ uint32_t genome_code(const AlignParams &ap, uint32_t pos)
{
	const uint32_t rel = pos - ap.sbo, byte = rel >> 2;
	if (byte >= ap.values_bytes) return 0u;
	return ((uint32_t)ap.values[byte] >> (2u * (rel & 3u))) & 3u;
}

// the 16 genome codes from pos on, LSB first
__device__ __forceinline__ uint32_t genome_word(const AlignParams &ap, uint32_t pos)
{
	const uint32_t rel = pos - ap.sbo, w = rel >> 4, sh = 2u * (rel & 15u);
	if (rel <= 0xffffffe0u && ((uint64_t)w + 2u) * 4u <= ap.values_bytes) {   // both words inside the image
		const uint32_t *g = (const uint32_t *)ap.values + w;
		return sh ? (g[0] >> sh) | (g[1] << (32u - sh)) : g[0];
	}
	uint32_t v = 0;
	for (uint32_t j = 0; j < 16u; j++) v |= genome_code(ap, pos + j) << (2u * j);
	return v;
}

// mask `which` := the read's codes against the genome at abs_pos + d + i
__device__ __forceinline__ void build_mask(const AlignParams &ap, AlignLds &S, int L, int which, uint32_t abs_pos, int d, int len)
{
	for (int w = 0; w < A_WORDS; w++) {
		uint32_t m = 0;
		if (16 * w < len) {
			const uint32_t x = S.rd[w][L] ^ genome_word(ap, abs_pos + (uint32_t)d + 16u * (uint32_t)w);
			m = (x | (x >> 1)) & 0x55555555u;
		}
		S.mk[which][w][L] = m;
	}
}

__device__ __forceinline__ int mask_bit(const AlignLds &S, int L, int which, int i)
{
	if (i < 0 || i >= 16 * A_WORDS) return 1;
	return (int)((S.mk[which][i >> 4][L] >> (2 * (i & 15))) & 1u);
}

// mismatches of bases [a, b) under mask `which`
__device__ __forceinline__ int mask_count(const AlignLds &S, int L, int which, int a, int b)
{
	if (a < 0) a = 0;
	if (b > 16 * A_WORDS) b = 16 * A_WORDS;
	int n = 0;
	for (int w = a >> 4; 16 * w < b; w++) {
		uint32_t m = S.mk[which][w][L];
		const int lo = a - 16 * w, hi = b - 16 * w;
		if (lo > 0) m &= 0xffffffffu << (2 * lo);
		if (hi < 16) m &= (1u << (2 * hi)) - 1u;
		n += __popc(m);
	}
	return n;
}

// base i of the read against the genome at abs_pos + d + i: from mask `which` where it holds offset
// md, else from the image (positions that wrapped: outside the reference's contract)
__device__ __forceinline__ int mism_at(const AlignParams &ap, const AlignLds &S, int L, int which, int md, uint32_t abs_pos, int d, int i)
{
	if (d == md) return mask_bit(S, L, which, i);
	if (i < 0 || i >= 16 * A_WORDS) return 1;
	return ((S.rd[i >> 4][L] >> (2 * (i & 15))) & 3u) != genome_code(ap, abs_pos + (uint32_t)d + (uint32_t)i);
}

__device__ __forceinline__ int subread_end(int len, int total, int subread)   // find_subread_end, input-files.c:1371-1377
{
	const int step = ((len << 16) - (19 << 16)) / (total - 1);
	return ((step * subread) >> 16) + 15;
}

// cellCounts_find_soft_clipping (:326-396) over mask `which`, whose base 0 is the scan's base -read_offset
__device__ __forceinline__ int soft_clipping(const AlignLds &S, int L, int which, int read_offset, int test_len, bool to_tail, int center)
{
	int in_window = 0, matched = 5, last_matched = -1;
	const int start = center < 0 ? 0 : center >= test_len ? test_len - 1 : to_tail ? center - 1 : center + 1;
	const int delta = to_tail ? 1 : -1;
	for (int a = start; a >= 0 && a < test_len; a += delta) {
		const int m = 1 - mask_bit(S, L, which, read_offset + a);
		matched += m;
		if (m) last_matched = a;
		in_window++;
		if (in_window > 5) matched -= 1 - mask_bit(S, L, which, read_offset + a - delta * 5);
		else matched--;
		if (matched < 4) {
			if (to_tail) return last_matched < 0 ? test_len - start : test_len - last_matched - 1;
			return last_matched >= 0 ? last_matched : start - 1;
		}
	}
	if (last_matched < 0) return test_len;
	return to_tail ? test_len - last_matched - 1 : last_matched;
}

// cellCounts_matchBin_chro (:2426-2458): matches of read bases [base_offset, + test_len) under the
// mask of their offset; 0 where the walk starts outside the image or reaches its end
__device__ __forceinline__ int match_bin(const AlignParams &ap, const AlignLds &S, int L, int which, int base_offset, uint32_t pos, int test_len)
{
	if (test_len <= 0) return 0;
	const uint32_t rel = pos - ap.sbo;
	if ((rel >> 2) >= ap.values_bytes) return 0;
	if ((uint64_t)(rel >> 2) + ((rel & 3u) + (uint32_t)test_len) / 4u >= ap.values_bytes) return 0;
	return test_len - mask_count(S, L, which, base_offset, base_offset + test_len);
}

// cellCounts_calculate_pos_weight_1sec (:1535-1548)
__device__ __forceinline__ int64_t weight_1sec(const AlignParams &ap, uint32_t pos, int len)
{
	if (!ap.planes || len <= 0) return 10;
	const uint32_t a = pos + 1u;
	uint32_t b = pos + (uint32_t)len;
	if (b < a || a >= ap.plane_bits) return 10;
	if (b >= ap.plane_bits) b = (uint32_t)(ap.plane_bits - 1u);
	const uint32_t pw = (uint32_t)(ap.plane_bits >> 5);
	bool flank = false;
	for (uint32_t w = a >> 5; w <= (b >> 5); w++) {
		uint32_t m = 0xffffffffu;
		if (w == (a >> 5)) m &= 0xffffffffu << (a & 31u);
		if (w == (b >> 5)) m &= 0xffffffffu >> (31u - (b & 31u));
		if (ap.planes[w] & m) return A_TOP;
		if (ap.planes[pw + w] & m) flank = true;
	}
	return flank ? 13 : 10;
}

// cellCounts_reduce_Cigar (:238-265) fed piece by piece, with cellCounts_calculate_pos_weight
// (:1550-1571) taken over its output as it comes
struct Cigar {
	char *out;
	int w, repeat, old, rlen;
	uint32_t pos;
	int64_t weight;
};

__device__ __forceinline__ void cigar_flush(const AlignParams &ap, Cigar &c)
{
	const int op = c.old, n = c.repeat;
	if (op == 'M' || op == 'S' || op == 'I') c.rlen += n;
	// "%d%c": at most 10 digits; the field holds every text of a record that is written (subread_vote.h)
	int k = 1;
	uint32_t top = 1;
	while ((uint32_t)n / top >= 10u) { top *= 10u; k++; }
	if (c.w >= 0 && c.w + k + 1 < SVG_CELL_CIGAR) {
		for (; top; top /= 10u) c.out[c.w++] = (char)('0' + (uint32_t)n / top % 10u);
		c.out[c.w++] = (char)op;
	} else c.w = -1;
	if (op == 'M') {
		if (c.weight < A_TOP) {
			const int64_t s = weight_1sec(ap, c.pos, n);
			if (s > c.weight) c.weight = s;
		}
		c.pos += (uint32_t)n;
	} else if (op == 'D' || op == 'N' || op == 'S') c.pos += (uint32_t)n;
	c.repeat = 0;
}

__device__ __forceinline__ void cigar_op(const AlignParams &ap, Cigar &c, int op, int n)
{
	if (c.old != op && c.repeat > 0) cigar_flush(ap, c);
	c.repeat += n;
	c.old = op;
}

// "%d<op>" as reduce_Cigar reads it: a '-' is an operation of count 1, then the digits
__device__ __forceinline__ void cigar_piece(const AlignParams &ap, Cigar &c, int n, int op)
{
	if (n < 0) { cigar_op(ap, c, '-', 1); n = -n; }
	cigar_op(ap, c, op, n);
}

__global__ void __launch_bounds__(64) align_explain_kernel(AlignParams ap)
{
	__shared__ AlignLds S;
	const int L = (int)threadIdx.x;
	const uint64_t t = (uint64_t)blockIdx.x * 64u + threadIdx.x;
	if (t >= (uint64_t)ap.cp.n * (uint64_t)ap.max_simples) return;
	const uint32_t c = (uint32_t)(t / ap.cp.n), r = (uint32_t)(t - (uint64_t)c * ap.cp.n);
	if (c >= ap.ncand[r]) return;
	const int len = ap.cp.lens[r], applied = ap.cp.heads[r].applied_subreads;
	const svg_cell_slot *sl = ap.cp.staging + (size_t)r * C_SLOTS + ap.cand[(size_t)c * ap.cp.n + r];
	svg_cell_aln *rec = ap.crec + (size_t)r * ap.max_simples + c;
	{
		uint4 *z = (uint4 *)rec;
#pragma unroll
		for (int q = 0; q < (int)(sizeof(svg_cell_aln) / 16); q++) z[q] = make_uint4(0u, 0u, 0u, 0u);
	}
	const bool neg = (sl->mask & C_NEG) != 0;
	// the read's codes, LSB first (read_bin, :3084-3106); an exception base is code 3 on both strands
	{
		const uint64_t base = cell_read_base(ap.cp, r);
		for (int w = 0; w < A_WORDS; w++) {
			uint32_t v = 0;
			if (16 * w < len) {
				const uint64_t k0 = base + 16u * (uint32_t)w;
				const uint32_t *bw = ap.cp.bases + (k0 >> 4);
				const uint32_t s2 = 2u * (uint32_t)(k0 & 15u);
				const uint32_t W = __builtin_bitreverse32(s2 ? (bw[0] << s2) | (bw[1] >> (32u - s2)) : bw[0]);
				v = ((W >> 1) & 0x55555555u) | ((W & 0x55555555u) << 1);
				uint32_t ex = 0;
				if (ap.cp.xmask) {
					const uint32_t *xw = ap.cp.xmask + (k0 >> 5);
					const uint32_t s1 = (uint32_t)(k0 & 31u);
					uint32_t e = __builtin_bitreverse32(s1 > 16u ? (xw[0] << s1) | (xw[1] >> (32u - s1)) : xw[0] << s1) & 0xffffu;
					e = (e | (e << 8)) & 0x00ff00ffu;
					e = (e | (e << 4)) & 0x0f0f0f0fu;
					e = (e | (e << 2)) & 0x33333333u;
					e = (e | (e << 1)) & 0x55555555u;
					ex = e | (e << 1);
				}
				if (neg) v = ~v | ex;
				else v |= ex;
				const int left = len - 16 * w;
				if (left < 16) v &= (1u << (2 * left)) - 1u;
			}
			(neg ? S.tmp : S.rd)[w][L] = v;
		}
		if (neg) {
			// reverse_read: base i = the complement of base len - 1 - i (tmp holds the complements, an
			// exception base 3).  Q = all 160 reversed, then down by 160 - len
			for (int w = 0; w < A_WORDS; w++) {
				const int s = 16 * A_WORDS - len + 16 * w;          // Q's base index of word w's base 0
				uint32_t v = 0;
				if (16 * w < len) {
					const int q = s >> 4, sh = 2 * (s & 15);
					// Q word q = word 9 - q, bases reversed
					uint32_t lo = 0, hi = 0;
					{
						const uint32_t f = S.tmp[A_WORDS - 1 - q][L], b = __builtin_bitreverse32(f);
						lo = ((b >> 1) & 0x55555555u) | ((b & 0x55555555u) << 1);
					}
					if (q + 1 < A_WORDS) {
						const uint32_t f = S.tmp[A_WORDS - 2 - q][L], b = __builtin_bitreverse32(f);
						hi = ((b >> 1) & 0x55555555u) | ((b & 0x55555555u) << 1);
					}
					v = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
					const int left = len - 16 * w;
					if (left < 16) v &= (1u << (2 * left)) - 1u;
				}
				S.rd[w][L] = v;
			}
		}
	}
	// cellCounts_indel_recorder_copy (:2352-2424)
	for (int i = 0; i < A_IND; i++) S.ind[i][L] = 0;
	const int tolimax = sl->toli;
	int move = 0;
	if (tolimax <= 3) {
		S.ind[0][L] = sl->indel_recorder[0];
		S.ind[1][L] = sl->indel_recorder[1];
	} else {
		for (int s = 0; s < applied; s++) S.off[s][L] = 0x77;
		for (int q = 0; q < tolimax; q += 3)
			for (int s = sl->indel_recorder[q]; s <= sl->indel_recorder[q + 1]; s++)
				if (s >= 1 && s <= applied) S.off[s - 1][L] = (int8_t)sl->indel_recorder[q + 2];
		for (int s = 0; s < applied; s++)
			if (S.off[s][L] != 0x77) { move = S.off[s][L]; break; }
		int cur = 0, subread0 = -1, q = 0;
		for (int s = 0;; s++) {
			int o = S.off[s][L];
			if (o != 0x77) {
				o = (int8_t)(o - move);
				S.off[s][L] = (int8_t)o;
				if (subread0 < 0) { subread0 = s + 1; cur = o; }
			}
			if (cur != o && subread0 > 0) {
				S.ind[q][L] = (int16_t)subread0;
				S.ind[q + 1][L] = (int16_t)s;
				S.ind[q + 2][L] = (int16_t)cur;
				cur = o;
				subread0 = s + 1;
				q += 3;
				if (q >= SVG_CELL_RECORDER) break;
				if (q + 3 < A_IND) S.ind[q + 3][L] = 0;   // (:2402 writes element 21 for q = 18, past the array; not here)
			}
			if (o == 0x77) subread0 = -1;
			if (s == applied - 1) {
				if (subread0 > 0) {
					S.ind[q][L] = (int16_t)subread0;
					S.ind[q + 1][L] = (int16_t)(s + 1);
					S.ind[q + 2][L] = (int16_t)cur;
					if (q + 3 < SVG_CELL_RECORDER) S.ind[q + 3][L] = 0;
				}
				break;
			}
		}
	}
	// cellCounts_explain_one_read (:2520-2627)
	const uint32_t abs_pos = sl->pos + (uint32_t)move;
	int in_cigar = 0, mism = 0, matched = 0, mapped = 0, all_indel = 0;
	int last_indel = S.ind[2][L], last_sub = S.ind[1][L] - 1, head = -1, last_mapped = 0;
	int cur = 0;                                         // the mask that holds offset last_indel
	build_mask(ap, S, L, cur, abs_pos, last_indel, len);
	Cigar cg;
	cg.out = rec->cigar; cg.w = 0; cg.repeat = 0; cg.old = 0; cg.rlen = 0; cg.pos = abs_pos; cg.weight = 10;
	for (int q = 3; q < tolimax; q += 3) {
		if (S.ind[q][L] == 0) break;
		const int v_first = S.ind[q][L] - 1, v_last = S.ind[q + 1][L] - 1, off = S.ind[q + 2][L], diff = off - last_indel;
		if (abs(diff) >= ap.p.max_indel_length) continue;
		int lcb = subread_end(len, applied, last_sub) - 8;
		const int fcb = subread_end(len, applied, v_first) - 16 + 8;
		if (lcb < in_cigar) lcb = in_cigar;
		uint32_t meet = abs_pos + (uint32_t)lcb + (uint32_t)last_indel;
		if (head < 0) {
			const int fm = subread_end(len, applied, S.ind[0][L] - 1);
			head = soft_clipping(S, L, cur, 0, fm, false, fm);
			if (head > 0) cigar_piece(ap, cg, head, 'S');
			if (meet < (uint32_t)head + abs_pos) meet = (uint32_t)head + abs_pos;
			if (head > lcb) lcb = head;
			in_cigar = head;
		}
		build_mask(ap, S, L, cur ^ 1, abs_pos, off, len);
		// cellCounts_meet_in_the_middle (:2462-2506).  A walk over the gap's bases through mism_at, on
		// purpose: two prefix popcounts of the masks would do, but mism_at also answers for a base
		// outside the mask's window or the array, the gap is at most a few dozen bases, and the whole
		// kernel is 2.3 ms of about 60 ms of kernel time (profiles/cellalign/bench_cellalign.json)
		const int gap = fcb - lcb, first = diff < 0 ? -diff : 0, d1 = (int)(meet - abs_pos) - lcb;
		int best = A_INVALID, max_matched = -99999;
		if (gap > first) {
			int fmt = 0, smt = 0;
			for (int x = first; x < gap; x++) smt += 1 - mism_at(ap, S, L, cur ^ 1, off, abs_pos, d1 + diff, lcb + x);
			for (int s = first; s < gap; s++) {
				if (fmt + smt > max_matched) { max_matched = fmt + smt; best = s; }
				fmt += 1 - mism_at(ap, S, L, cur, last_indel, abs_pos, d1, lcb + s - first);
				smt -= 1 - mism_at(ap, S, L, cur ^ 1, off, abs_pos, d1 + diff, lcb + s);
			}
		}
		const int gap_mm = gap - max_matched + (diff < 0 ? diff : 0);
		int ipos = best + (diff < 0 ? diff : 0);
		if (best == A_INVALID) { ipos = gap / 2; all_indel += abs(diff); }
		const int sec = match_bin(ap, S, L, cur, in_cigar, abs_pos + (uint32_t)in_cigar + (uint32_t)last_indel, lcb - in_cigar);
		mism += gap_mm + (lcb - in_cigar - sec);
		matched += sec + fcb - lcb - gap_mm + (diff < 0 ? diff : 0);
		cigar_piece(ap, cg, lcb - in_cigar, 'M');
		cigar_piece(ap, cg, ipos, 'M');
		cigar_piece(ap, cg, abs(diff), diff > 0 ? 'D' : 'I');
		cigar_piece(ap, cg, fcb - lcb - ipos + (diff < 0 ? diff : 0), 'M');
		mapped += fcb - in_cigar + (diff < 0 ? diff : 0);
		in_cigar = fcb;
		last_mapped = subread_end(len, applied, v_last) - 16 + 9;
		last_indel = off;
		last_sub = v_last;
		cur ^= 1;
	}
	if (head < 0) {
		const int fm = subread_end(len, applied, S.ind[0][L] - 1) - 8;
		head = soft_clipping(S, L, cur, 0, fm, false, fm);
		if (head > 0) cigar_piece(ap, cg, head, 'S');
		in_cigar = head;
		last_mapped = subread_end(len, applied, last_sub) - 16 + 8;
	}
	const int tail = soft_clipping(S, L, cur, last_mapped, len - last_mapped, true, 1);
	const int sec = match_bin(ap, S, L, cur, in_cigar, abs_pos + (uint32_t)in_cigar + (uint32_t)last_indel, len - in_cigar - tail);
	mism += len - in_cigar - tail - sec;
	matched += sec;
	cigar_piece(ap, cg, len - in_cigar - tail, 'M');
	mapped += len - in_cigar - tail;
	if (tail) cigar_piece(ap, cg, tail, 'S');
	if (cg.repeat > 0) cigar_flush(ap, cg);
	int64_t score = 0;
	if (cg.rlen == len && mapped >= ap.p.min_mapped_length_for_mapped_read && mism <= ap.p.max_mismatching_bases_in_reads)
		score = (int64_t)((uint64_t)(int64_t)matched * 1000000ull / (1ull + (uint64_t)(int64_t)mism)) * cg.weight;   // cellCounts_test_score
	// a text past the field: no record that is written has one (subread_vote.h); counted, and the call fails
	if (cg.w < 0) { if (score > 0) atomicAdd(ap.overflow, 1u); score = 0; }
	rec->score = score;
	rec->position = abs_pos;
	rec->flags = neg ? 16 : 0;
	rec->mapq = (int16_t)(40 - mism);
	rec->editing_distance = mism + all_indel;
}

__global__ void __launch_bounds__(64) align_emit_kernel(AlignParams ap)
{
	__shared__ uint8_t s_ord[SVG_CELL_MAX_REPORT][64];
	__shared__ uint16_t s_stk[A_STACK][64];
	const int L = (int)threadIdx.x;
	const uint32_t r = blockIdx.x * 64u + threadIdx.x;
	if (r >= ap.cp.n) return;
	const int count = ap.ncand[r];
	const svg_cell_aln *rec = ap.crec + (size_t)r * ap.max_simples;
	int multi = 0, nrec = 0;
	for (int i = 0; i < count; i++) {
		if (rec[i].score > 0) multi++;
		s_ord[i][L] = (uint8_t)i;
	}
	if (multi > ap.p.max_reported_alignments_per_read) multi = ap.p.max_reported_alignments_per_read;
	if (multi) {
		// quick_sort_run (core.c:4694-4714) with sort_readscore_compare_LargeFirst (:2629-2638)
		int lo = 0, hi = count - 1, sp = 0;
		for (;;) {
			int i = lo - 1;
			{
				const int64_t pv = rec[s_ord[hi][L]].score;
				for (int j = lo; j < hi; j++) {
					const uint8_t oj = s_ord[j][L];
					if (rec[oj].score >= pv) {
						i++;
						s_ord[j][L] = s_ord[i][L];
						s_ord[i][L] = oj;
					}
				}
				const uint8_t tt = s_ord[i + 1][L];
				s_ord[i + 1][L] = s_ord[hi][L];
				s_ord[hi][L] = tt;
			}
			const bool left = i > lo, right = hi > i + 2;
			if (left && right) {
				if (i - lo + 1 >= hi - i - 1) { s_stk[sp++][L] = (uint16_t)(lo | (i << 8)); lo = i + 2; }
				else { s_stk[sp++][L] = (uint16_t)((i + 2) | (hi << 8)); hi = i; }
			} else if (left) hi = i;
			else if (right) lo = i + 2;
			else {
				if (!sp) break;
				const uint16_t e = s_stk[--sp][L];
				lo = e & 255;
				hi = e >> 8;
			}
		}
		for (int a = 0; a < multi; a++) {
			const int myno = s_ord[a][L];
			if (rec[myno].score < 1) continue;
			if (a >= ap.p.max_reported_alignments_per_read) break;
			ap.order[(size_t)nrec++ * ap.cp.n + r] = (uint8_t)myno;
		}
	}
	uint32_t *hw = (uint32_t *)(ap.aheads + r);
	hw[0] = 0; hw[1] = 0;
	hw[2] = (uint32_t)nrec | ((uint32_t)multi << 16);
	hw[3] = 0;
}

// aheads[r].first_record = rec_base + (records of the chunk's reads before r) for a read with records
__global__ void __launch_bounds__(1024) align_scan_kernel(AlignParams ap)
{
	__shared__ uint32_t part[1024];
	const uint32_t tid = threadIdx.x, n = ap.cp.n, per = (n + 1023u) / 1024u;
	const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
	uint32_t sum = 0;
	for (uint32_t r = lo; r < hi; r++) sum += ap.aheads[r].n_records;
	part[tid] = sum;
	__syncthreads();
	for (uint32_t d = 1; d < 1024u; d <<= 1) {
		const uint32_t v = tid >= d ? part[tid - d] : 0u;
		__syncthreads();
		part[tid] += v;
		__syncthreads();
	}
	uint64_t at = ap.rec_base + (part[tid] - sum);
	for (uint32_t r = lo; r < hi; r++) {
		if (ap.aheads[r].n_records) ap.aheads[r].first_record = at;
		at += ap.aheads[r].n_records;
	}
	if (tid == 1023u) *ap.total = part[1023];
}

// thread = (record k, read): the chosen candidate's record to its place
__global__ void __launch_bounds__(256) align_compact_kernel(AlignParams ap)
{
	const uint64_t total = (uint64_t)ap.cp.n * (uint64_t)ap.p.max_reported_alignments_per_read;
	for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256u) {
		const uint32_t k = (uint32_t)(t / ap.cp.n), r = (uint32_t)(t - (uint64_t)k * ap.cp.n);
		const svg_cell_aln_head *h = ap.aheads + r;
		if (k >= h->n_records) continue;
		const uint4 *src = (const uint4 *)(ap.crec + (size_t)r * ap.max_simples + ap.order[(size_t)k * ap.cp.n + r]);
		uint4 *dst = (uint4 *)(ap.compact + (h->first_record - ap.rec_base + k));
#pragma unroll
		for (int q = 0; q < (int)(sizeof(svg_cell_aln) / 16); q++) dst[q] = src[q];
	}
}

// thread = interval: the exon plane and the flank plane (:938-959); bits at and past plane_bits are dropped
__global__ void __launch_bounds__(256) align_exon_kernel(const uint32_t *starts, const uint32_t *stops, uint64_t n, uint32_t *planes,
                                                         uint64_t plane_bits)
{
	const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (e >= n) return;
	const uint32_t a0 = starts[e], b0 = stops[e];
	if (a0 > 0xffffff00u || b0 > 0xffffff00u) return;   // :941
	for (int pl = 0; pl < 2; pl++) {
		// (the flank loop's start is unsigned: below 100 it wraps past the stop and sets nothing)
		const uint32_t a = pl ? a0 - 100u : a0;
		uint32_t b = pl ? b0 + 100u : b0;
		if (a > b || a >= plane_bits) continue;
		if (b >= plane_bits) b = (uint32_t)(plane_bits - 1u);
		uint32_t *p = planes + (size_t)pl * (size_t)(plane_bits >> 5);
		for (uint32_t w = a >> 5; w <= (b >> 5); w++) {
			uint32_t m = 0xffffffffu;
			if (w == (a >> 5)) m &= 0xffffffffu << (a & 31u);
			if (w == (b >> 5)) m &= 0xffffffffu >> (31u - (b & 31u));
			atomicOr(p + w, m);
		}
	}
}

extern "C" void svg_cell_align_params_default(svg_cell_align_params *p)
{
	if (!p) return;
	p->total_subreads = 10;                          // cell-counts.c:526
	p->max_indel_length = 5;                         // :521
	p->min_votes_per_mapped_read = 3;                // :525
	p->max_differential_from_top_vote_number = 2;    // :524
	p->max_mismatching_bases_in_reads = 3;           // :519
	p->min_mapped_length_for_mapped_read = 40;       // :529
	p->max_reported_alignments_per_read = 1;         // :517
}

extern "C" void svg_cell_align_free(svg_cell_alns *res)
{
	if (!res) return;
	free(res->heads);
	free(res->alns);
	memset(res, 0, sizeof *res);
}

static_assert(sizeof(svg_cell_aln_head) == 16 && sizeof(svg_cell_aln) == 128, "svg_cell_aln record layout");

static uint64_t exon_plane_bits(const svg_index *h)
{
	uint64_t bits = (uint64_t)h->dix.start_base_offset + 4ull * h->dix.values_bytes + SVG_CELL_EXON_TAIL;
	if (bits > (1ull << 32)) bits = 1ull << 32;
	return (bits + 31u) & ~31ull;
}

extern "C" int svg_cell_set_exons(svg_index *h, const uint32_t *starts, const uint32_t *stops, uint64_t n)
{
	if (!h || (n && (!starts || !stops))) { svg_set_error("svg_cell_set_exons: NULL argument"); return SVG_E_ARG; }
	if (h->nblocks > 1) {
		svg_set_error("svg_cell_set_exons: an index of %d blocks (cellCounts takes a one-block index)", h->nblocks);
		return SVG_E_UNSUPPORTED;
	}
	for (uint64_t e = 0; e < n; e++)
		if (starts[e] > stops[e]) {
			svg_set_error("svg_cell_set_exons: interval %llu ends before it starts", (unsigned long long)e);
			return SVG_E_ARG;
		}
	HIPCHK(hipSetDevice(h->device));
	hipStream_t st = h->stream;
	if (h->last_pending) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));
	HIPCHK(hipStreamSynchronize(st));
	if (!n) {
		if (h->d_exons) { hipFree(h->d_exons); h->d_exons = NULL; h->device_bytes -= (size_t)(exon_plane_bits(h) / 8) * 2; }
		return 0;
	}
	const uint64_t bits = exon_plane_bits(h);
	const size_t bytes = (size_t)(bits / 8) * 2;
	int rc;
	if (!h->d_exons && (rc = dmalloc(h, (void **)&h->d_exons, bytes))) return rc;
	void *d = NULL;
	if ((rc = dmalloc(h, &d, 8 * n))) return rc;
	h->device_bytes -= 8 * n;
	hipError_t e = hipMemsetAsync(h->d_exons, 0, bytes, st);
	if (e == hipSuccess) e = hipMemcpyAsync(d, starts, 4 * n, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = hipMemcpyAsync((uint32_t *)d + n, stops, 4 * n, hipMemcpyHostToDevice, st);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(align_exon_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint32_t *)d,
		                   (const uint32_t *)d + n, n, h->d_exons, bits);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	hipFree(d);
	if (e != hipSuccess) { svg_set_error("svg_cell_set_exons: HIP error %s", hipGetErrorString(e)); return SVG_E_DEVICE; }
	return 0;
}

static int align_params_check(const svg_cell_align_params *p, const char *who)
{
	struct { const char *name; int v, lo, hi; } f[] = {
		{"total_subreads", p->total_subreads, 7, C_SUB},                                              // :547
		{"max_indel_length", p->max_indel_length, 5, 5},                                              // :521
		{"min_votes_per_mapped_read", p->min_votes_per_mapped_read, 1, 64},                           // :544
		{"max_differential_from_top_vote_number", p->max_differential_from_top_vote_number, 1, 30},   // :556
		{"max_mismatching_bases_in_reads", p->max_mismatching_bases_in_reads, 0, 100},                // :538
		{"min_mapped_length_for_mapped_read", p->min_mapped_length_for_mapped_read, -1, SVG_CELL_MAX_READ_LENGTH},   // :541
		{"max_reported_alignments_per_read", p->max_reported_alignments_per_read, 1, SVG_CELL_MAX_REPORT},           // :569
	};
	for (size_t i = 0; i < sizeof f / sizeof f[0]; i++)
		if (f[i].v < f[i].lo || f[i].v > f[i].hi) {
			svg_set_error("%s: %s %d outside %d..%d", who, f[i].name, f[i].v, f[i].lo, f[i].hi);
			return SVG_E_ARG;
		}
	return 0;
}

extern "C" int svg_cell_align_batch(svg_index *h, const svg_cell_align_params *p, const svg_packed_reads *reads, svg_cell_alns *res)
{
	return cell_align_run(h, p, reads, res, NULL, NULL, NULL);
}

int cell_align_run(svg_index *h, const svg_cell_align_params *p, const svg_packed_reads *reads, svg_cell_alns *res,
                   const svg_packed_reads *bc, svg_cell_hits *hits, int32_t **barcode_no, CellCountSink *sink, bool quiet)
{
	const char *who = sink ? cell_count_who(sink) : hits ? "svg_cell_assign_batch" : "svg_cell_align_batch";   // the entry point named in error texts
	if (!h || !p || !reads || !res) { svg_set_error("%s: NULL argument", who); return SVG_E_ARG; }
	memset(res, 0, sizeof *res);
	if (h->nblocks > 1) {
		svg_set_error("%s: an index of %d blocks (cellCounts takes a one-block index)", who, h->nblocks);
		return SVG_E_UNSUPPORTED;
	}
	int rc = align_params_check(p, who);
	if (rc) return rc;
	if (h->dix.start_base_offset & 3u) {
		svg_set_error("%s: an .array image that starts at base %u (not a multiple of 4)", who, h->dix.start_base_offset);
		return SVG_E_UNSUPPORTED;
	}
	const uint64_t n = reads->n_reads;
	if (n == 0) return 0;
	if (!reads->bases || !reads->lens) { svg_set_error("%s: NULL read buffer", who); return SVG_E_ARG; }
	uint64_t nbases = 0;
	for (uint64_t r = 0; r < n; r++) {
		if (reads->lens[r] > SVG_CELL_MAX_READ_LENGTH) {
			svg_set_error("%s: read %llu has %d bases (at most %d)", who, (unsigned long long)r, (int)reads->lens[r],
			              SVG_CELL_MAX_READ_LENGTH);
			return SVG_E_ARG;
		}
		if (!reads->starts && reads->lens[r] > reads->stride) {
			svg_set_error("%s: read %llu is longer than the stride", who, (unsigned long long)r);
			return SVG_E_ARG;
		}
		const uint64_t e = (reads->starts ? reads->starts[r] : r * reads->stride) + reads->lens[r];
		if (e > nbases) nbases = e;
	}
	HIPCHK(hipSetDevice(h->device));
	hipStream_t st = h->stream;
	if (h->last_pending) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));
	const uint64_t CH = 1u << 17;   // reads per chunk: 51 staging records and max_voting_simples candidate records each
	const uint64_t m = n < CH ? n : CH;
	const int S = p->max_reported_alignments_per_read > 3 ? p->max_reported_alignments_per_read : 3;   // :518, :604
	const int R = p->max_reported_alignments_per_read;
	const size_t bw = (size_t)((nbases + 15) / 16) * 4, xw = reads->xmask ? (size_t)((nbases + 31) / 32) * 4 : 0;
	enum { D_BASES, D_XMASK, D_STARTS, D_LENS, D_PROBES, D_HEADS, D_STAGING, D_CAND, D_NCAND, D_CREC, D_ORDER, D_AHEADS, D_COMPACT,
	       D_TOTAL, D_N };
	size_t sizes[D_N];
	sizes[D_BASES] = bw + 8; sizes[D_XMASK] = xw + 8; sizes[D_STARTS] = reads->starts ? 8 * n : 0; sizes[D_LENS] = 2 * n;
	sizes[D_PROBES] = sizeof(uint2) * 2 * C_SUB * m; sizes[D_HEADS] = sizeof(svg_cell_head) * m;
	sizes[D_STAGING] = sizeof(svg_cell_slot) * C_SLOTS * m; sizes[D_CAND] = (size_t)S * m; sizes[D_NCAND] = m;
	sizes[D_CREC] = sizeof(svg_cell_aln) * S * m; sizes[D_ORDER] = (size_t)R * m; sizes[D_AHEADS] = sizeof(svg_cell_aln_head) * m;
	sizes[D_COMPACT] = sizeof(svg_cell_aln) * R * m; sizes[D_TOTAL] = 16;
	void *d[D_N];
	memset(d, 0, sizeof d);
	uint64_t held = 0, nrec = 0, cap = 0;
	for (int i = 0; i < D_N && !rc; i++) {
		if (!sizes[i]) continue;
		if (!(rc = dmalloc(h, &d[i], sizes[i]))) held += sizes[i];
	}
	if (!quiet) res->heads = (svg_cell_aln_head *)malloc(sizeof(svg_cell_aln_head) * n);
	if (!rc && !quiet && !res->heads) { svg_set_error("out of host memory"); rc = SVG_E_NOMEM; }
	if (!rc && (hipMemcpyAsync(d[D_BASES], reads->bases, bw, hipMemcpyHostToDevice, st) != hipSuccess ||
	            hipMemsetAsync((char *)d[D_BASES] + bw, 0, 8, st) != hipSuccess ||
	            (xw && hipMemcpyAsync(d[D_XMASK], reads->xmask, xw, hipMemcpyHostToDevice, st) != hipSuccess) ||
	            (xw && hipMemsetAsync((char *)d[D_XMASK] + xw, 0, 8, st) != hipSuccess) ||
	            (reads->starts && hipMemcpyAsync(d[D_STARTS], reads->starts, 8 * n, hipMemcpyHostToDevice, st) != hipSuccess) ||
	            hipMemcpyAsync(d[D_LENS], reads->lens, 2 * n, hipMemcpyHostToDevice, st) != hipSuccess)) {
		svg_set_error("%s: upload failed", who);
		rc = SVG_E_DEVICE;
	}
	if (!rc && hipMemsetAsync(d[D_TOTAL], 0, 16, st) != hipSuccess) { svg_set_error("%s: upload failed", who); rc = SVG_E_DEVICE; }
	// svg_set_timing: events around each launch, summed per kernel (svg_cell_align_timing)
	hipEvent_t ev[7] = {NULL, NULL, NULL, NULL, NULL, NULL, NULL};
	if (!rc && h->timing)
		for (int i = 0; i < 7; i++)
			if (hipEventCreate(&ev[i]) != hipSuccess) { svg_set_error("%s: hipEventCreate failed", who); rc = SVG_E_DEVICE; break; }
	const int img = key_image(h);
	CellAssignRun *run = NULL;
	if (!rc && hits) rc = cell_assign_begin(h, bc, n, m, R, st, &run, quiet, sink && cell_count_has_names(sink));
	if (!rc && sink) rc = cell_count_begin(sink, n, m, st);
	for (uint64_t o = 0; o < n && !rc; o += m) {
		const uint64_t k = n - o < m ? n - o : m;
		AlignParams ap;
		memset(&ap, 0, sizeof ap);
		CellParams &cp = ap.cp;
		cp.kt = key_table(h);
		cp.vals = h->dix.vals;
		cp.gap = h->dix.gap;
		cp.total_subreads = p->total_subreads;
		cp.max_indel = p->max_indel_length;
		cp.bases = (const uint32_t *)d[D_BASES];
		cp.xmask = xw ? (const uint32_t *)d[D_XMASK] : NULL;
		cp.starts = reads->starts ? (const uint64_t *)d[D_STARTS] + o : NULL;
		cp.stride = reads->stride;
		cp.base0 = o * reads->stride;
		cp.lens = (const uint16_t *)d[D_LENS] + o;
		cp.n = (uint32_t)k;
		cp.probes = (uint2 *)d[D_PROBES];
		cp.heads = (svg_cell_head *)d[D_HEADS];
		cp.staging = (svg_cell_slot *)d[D_STAGING];
		ap.p = *p;
		ap.max_simples = S;
		ap.values = h->dix.values;
		ap.values_bytes = h->dix.values_bytes;
		ap.sbo = h->dix.start_base_offset;
		ap.planes = h->d_exons;
		ap.plane_bits = h->d_exons ? exon_plane_bits(h) : 0;
		ap.cand = (uint8_t *)d[D_CAND];
		ap.ncand = (uint8_t *)d[D_NCAND];
		ap.crec = (svg_cell_aln *)d[D_CREC];
		ap.order = (uint8_t *)d[D_ORDER];
		ap.aheads = (svg_cell_aln_head *)d[D_AHEADS];
		ap.compact = (svg_cell_aln *)d[D_COMPACT];
		ap.rec_base = nrec;
		ap.total = (uint64_t *)d[D_TOTAL];
		ap.overflow = (uint32_t *)d[D_TOTAL] + 2;
		if (ev[0]) hipEventRecord(ev[0], st);
		cell_launch_vote(cp, img, h->n_cu, st, ev[1]);
		if (ev[2]) hipEventRecord(ev[2], st);
		uint64_t cblocks = (k * R + 255) / 256;
		if (cblocks > (uint64_t)h->n_cu * 16) cblocks = (uint64_t)h->n_cu * 16;
		hipLaunchKernelGGL(align_select_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, ap);
		if (ev[3]) hipEventRecord(ev[3], st);
		hipLaunchKernelGGL(align_explain_kernel, dim3((unsigned)((k * S + 63) / 64)), dim3(64), 0, st, ap);
		if (ev[4]) hipEventRecord(ev[4], st);
		hipLaunchKernelGGL(align_emit_kernel, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, st, ap);
		if (ev[5]) hipEventRecord(ev[5], st);
		hipLaunchKernelGGL(align_scan_kernel, dim3(1), dim3(1024), 0, st, ap);
		hipLaunchKernelGGL(align_compact_kernel, dim3((unsigned)cblocks), dim3(256), 0, st, ap);
		if (ev[6]) hipEventRecord(ev[6], st);
		uint64_t tot[2] = {0, 0};
		if (hipGetLastError() != hipSuccess ||
		    (!quiet && hipMemcpyAsync(res->heads + o, d[D_AHEADS], sizeof(svg_cell_aln_head) * k, hipMemcpyDeviceToHost, st) != hipSuccess) ||
		    hipMemcpyAsync(tot, d[D_TOTAL], 16, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
			svg_set_error("%s: HIP error %s", who, hipGetErrorString(hipGetLastError()));
			rc = SVG_E_DEVICE;
			break;
		}
		const uint64_t used = tot[0];
		if (tot[1]) {
			svg_set_error("%s: %llu CIGAR texts longer than SVG_CELL_CIGAR", who, (unsigned long long)(uint32_t)tot[1]);
			rc = SVG_E_DEVICE;
			break;
		}
		if (ev[0])
			for (int i = 0; i < 6; i++) {
				float ms = 0;
				if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) h->cell_ms[i] += ms;
			}
		if (!quiet && nrec + used > cap) {
			cap = nrec + used + used * ((n - o - k + k - 1) / k);
			svg_cell_aln *g = (svg_cell_aln *)realloc(res->alns, sizeof(svg_cell_aln) * cap);
			if (!g) { svg_set_error("out of host memory"); rc = SVG_E_NOMEM; break; }
			res->alns = g;
		}
		if (!quiet && used && hipMemcpy(res->alns + nrec, d[D_COMPACT], sizeof(svg_cell_aln) * used, hipMemcpyDeviceToHost) != hipSuccess) {
			svg_set_error("%s: download failed", who);
			rc = SVG_E_DEVICE;
			break;
		}
		const uint32_t *d_bcb = NULL, *d_bcx = NULL;
		if (sink && (rc = cell_count_parse(sink, o, k, &d_bcb, &d_bcx))) break;
		if (run && (rc = cell_assign_chunk(run, o, k, (const svg_cell_aln *)d[D_COMPACT], used, d_bcb, d_bcx))) break;
		if (sink) {
			const svg_cell_hit *d_hits;
			const int32_t *d_genes, *d_bc;
			uint64_t gene_base, n_genes;
			cell_assign_view(run, &d_hits, &d_genes, &gene_base, &n_genes, &d_bc);
			if ((rc = cell_count_chunk(sink, o, k, (const svg_cell_aln_head *)d[D_AHEADS], nrec, d_hits, d_genes, gene_base, n_genes, d_bc, st))) break;
		}
		nrec += used;
	}
	if (run) cell_assign_end(run, rc || quiet ? NULL : hits, rc || quiet ? NULL : barcode_no);
	for (int i = 0; i < D_N; i++) hipFree(d[i]);
	for (int i = 0; i < 7; i++)
		if (ev[i]) hipEventDestroy(ev[i]);
	h->device_bytes -= held;
	if (rc) { svg_cell_align_free(res); return rc; }
	if (quiet) return 0;
	res->n_reads = n;
	res->n_records = nrec;
	return 0;
}

extern "C" int svg_cell_align_timing(svg_index *h, double ms[6])
{
	if (!h || !ms) { svg_set_error("svg_cell_align_timing: NULL argument"); return SVG_E_ARG; }
	for (int i = 0; i < 6; i++) { ms[i] = h->cell_ms[i]; h->cell_ms[i] = 0; }
	return 0;
}
