/* TEST INFRASTRUCTURE ONLY: cellCounts' per-read step after the vote, restated in plain C in
 * svg_cell_align_batch's record format (include/subread_vote.h).  The vote itself is
 * cellvote_model.c's vote_read (included below); nothing is shared with the HIP.  Reference
 * lines (Subread v2.0.6):
 *   cellCounts_select_and_write_alignments  cell-counts.c:2648-2719
 *   cellCounts_update_top_three             cell-counts.c:2296-2310
 *   cellCounts_explain_one_read             cell-counts.c:2520-2627
 *   cellCounts_indel_recorder_copy          cell-counts.c:2352-2424
 *   cellCounts_find_soft_clipping           cell-counts.c:326-396
 *   cellCounts_meet_in_the_middle           cell-counts.c:2462-2506
 *   cellCounts_matchBin_chro                cell-counts.c:2426-2458
 *   cellCounts_test_score                   cell-counts.c:2508-2511
 *   cellCounts_calculate_pos_weight, _1sec  cell-counts.c:1535-1571
 *   cellCounts_reduce_Cigar                 cell-counts.c:238-265
 *   the exon planes                         cell-counts.c:938-959
 *   find_subread_end                        input-files.c:1371-1377
 *   quick_sort, quick_sort_run              core.c:4690-4714
 * The CIGAR is built at character level, as the reference builds it.  Reads are ASCII here.
 * Built as a shared object by tests/cellalign_common.py and, under the sanitizers, into the
 * stand-alone tests/native/cellalign_check.c. */
#include <stdio.h>
#include "cellvote_model.c"

#define TOLERANCE 7            /* MAX_INDEL_TOLERANCE, subread.h:225 */
#define REV_OFFSET (MAXLEN / 4 + 1)   /* REVERSED_READ_BIN_OFFSET, cell-counts.c:2513 */
#define MAX_REPORT 30          /* SCRNA_HIGHEST_REPORTED_ALIGNMENTS, subread.h:37 */
#define WEIGHT_TOP 10000000ll  /* SCORING_MAX_QUALITY_MAPPING, cell-counts.c:1533 */
#define INVALID_INDEL (-9999999)
#define CIGAR_FIELD 108        /* SVG_CELL_CIGAR */
#define EXON_TAIL 512          /* SVG_CELL_EXON_TAIL */

typedef struct {               /* svg_cell_align_params */
	int32_t total_subreads, max_indel_length, min_votes_per_mapped_read, max_differential_from_top_vote_number,
	        max_mismatching_bases_in_reads, min_mapped_length_for_mapped_read, max_reported_alignments_per_read;
} aparams_t;

typedef struct {               /* svg_cell_aln_head */
	uint64_t first_record;
	uint16_t n_records, multi_alignment_no;
	uint32_t pad;
} ahead_t;

typedef struct {               /* svg_cell_aln */
	int64_t score;
	uint32_t position;
	int16_t flags, mapq;
	int32_t editing_distance;
	char cigar[CIGAR_FIELD];
} aln_t;

typedef struct {
	const uint8_t *values;     /* the .array image */
	uint32_t values_bytes, start_base_offset;
	const uint8_t *planes;     /* two bit planes of plane_bits bits each, or NULL: no exons */
	uint64_t plane_bits;
	aparams_t p;
	int max_voting_simples;
	uint64_t outside;          /* genome bases asked outside the image */
	uint64_t overrun;          /* indel_recorder_copy's write one past its array (:2402) */
	uint32_t edges;            /* EDGE_* of the read in hand */
} actx_t;

/* edges of a read that its records do not show (tests/test_cellalign_golden.py) */
#define EDGE_ZERO_MM   1   /* a candidate scored 0 for its mismatches */
#define EDGE_ZERO_RLEN 2   /* a candidate scored 0 for rebuilt_rlen != read_len */
#define EDGE_TIE       4   /* two candidates share the top score, which is > 0 */
#define EDGE_W13       8   /* a candidate with a score > 0 at weight 13 */
#define EDGE_WTOP      16  /* a candidate with a score > 0 at weight 10^7 */

/* cellCounts_get_index_int with the library's rule for a base outside the image: code 0 */
static int genome_code(actx_t *c, unsigned int pos)
{
	const unsigned int byte = (pos - c->start_base_offset) >> 2;
	if (byte >= c->values_bytes) { c->outside++; return 0; }
	return (c->values[byte] >> (pos % 4 * 2)) & 3;
}

static int read_code(const char *bin, int off) { return (bin[off / 4] >> (off % 4 * 2)) & 3; }

static int subread_end(int len, int total, int subread)
{
	const int step = ((len << 16) - (19 << 16)) / (total - 1);
	return ((step * subread) >> 16) + 15;
}

static int soft_clipping(actx_t *c, const char *bin, int read_offset, unsigned int mapped_pos, int test_len, int to_tail,
                         int center)
{
	int in_window = 0, start, matched = 5, last_matched = -1, delta;
	if (to_tail) { start = center < 0 ? 0 : center >= test_len ? test_len - 1 : center - 1; delta = 1; }
	else { start = center < 0 ? 0 : center >= test_len ? test_len - 1 : center + 1; delta = -1; }
	for (int a = start; a >= 0 && a < test_len; a += delta) {
		const int m = genome_code(c, a + mapped_pos) == read_code(bin, read_offset + a);
		matched += m;
		if (m) last_matched = a;
		in_window++;
		if (in_window > 5) {
			const int r = a - delta * 5;
			matched -= genome_code(c, r + mapped_pos) == read_code(bin, r + read_offset);
		} else matched--;
		if (matched < 5 - 1) {
			if (to_tail) return last_matched < 0 ? test_len - start : test_len - last_matched - 1;
			return last_matched >= 0 ? last_matched : start - 1;
		}
	}
	if (last_matched < 0) return test_len;
	return to_tail ? test_len - last_matched - 1 : last_matched;
}

static int match_bin(actx_t *c, const char *bin, int base_offset, unsigned int pos, int test_len)
{
	unsigned int byte = (pos - c->start_base_offset) >> 2, bit = pos % 4 * 2;
	if (byte >= c->values_bytes) return 0;
	int ret = 0;
	for (int i = 0; i < test_len; i++) {
		if (((c->values[byte] >> bit) & 3) == read_code(bin, base_offset + i)) ret++;
		bit += 2;
		if (bit == 8) {
			byte++;
			if (byte == c->values_bytes) return 0;
			bit = 0;
		}
	}
	return ret;
}

static int meet_in_the_middle(actx_t *c, unsigned int first_pos, const char *bin, int bin_base, int gap, int indel,
                              int *gap_mismatch)
{
	unsigned short first_half[MAXLEN + 1], second_half[MAXLEN + 1];
	int best = INVALID_INDEL, max_matched = -99999, sum = 0;
	if (gap > MAXLEN) gap = MAXLEN;   /* (a gap is a distance inside the read) */
	for (int x = 0; x < gap; x++) {
		first_half[x] = (unsigned short)sum;
		sum += genome_code(c, first_pos + x) == read_code(bin, bin_base + x);
	}
	sum = 0;
	const int first = indel < 0 ? -indel : 0;
	for (int x = gap - 1; x >= first; x--) {
		sum += genome_code(c, first_pos + x + indel) == read_code(bin, bin_base + x);
		second_half[x] = (unsigned short)sum;
	}
	for (int s = first; s < gap; s++) {
		const int here = first_half[s - first] + second_half[s];
		if (here > max_matched) { max_matched = here; best = s; }
	}
	*gap_mismatch = gap - max_matched + (indel < 0 ? indel : 0);
	return best + (indel < 0 ? indel : 0);
}

static int recorder_copy(actx_t *c, int16_t *aln, const int16_t *vot, int tolimax, int applied, int *move)
{
	if (tolimax <= 3) { aln[0] = vot[0]; aln[1] = vot[1]; aln[2] = 0; aln[3] = 0; return 0; }
	char offsets[40];
	memset(offsets, 0x77, (size_t)applied);
	for (int t = 0; t < tolimax; t += 3)
		for (int s = vot[t]; s <= vot[t + 1]; s++) offsets[s - 1] = (char)vot[t + 2];
	for (int s = 0; s < applied; s++)
		if (offsets[s] != 0x77) { *move = offsets[s]; break; }
	int cur = 0, subread0 = -1, high = 0, t = 0;
	for (int s = 0;; s++) {
		if (offsets[s] != 0x77) {
			offsets[s] = (char)(offsets[s] - *move);
			if (subread0 < 0) { subread0 = s + 1; cur = offsets[s]; }
			high = offsets[s];
		}
		if (cur != offsets[s] && subread0 > 0) {
			aln[t] = (int16_t)subread0;
			aln[t + 1] = (int16_t)s;
			aln[t + 2] = (int16_t)cur;
			cur = offsets[s];
			subread0 = s + 1;
			t += 3;
			if (t >= TOLERANCE * 3) break;
			if (t + 3 >= TOLERANCE * 3) c->overrun++;   /* the reference writes alnrec[21] */
			aln[t + 3] = 0;
		}
		if (offsets[s] == 0x77) subread0 = -1;
		if (s == applied - 1) {
			if (subread0 > 0) {
				aln[t] = (int16_t)subread0;
				aln[t + 1] = (int16_t)(s + 1);
				aln[t + 2] = (int16_t)cur;
				if (t + 3 < TOLERANCE * 3) aln[t + 3] = 0;
				t += 3;
			}
			break;
		}
	}
	return high;
}

static int reduce_cigar(const char *cigar, char *out)
{
	int tmpi = -1, repeat = 0, old = 0, w = 0, rlen = 0;
	out[0] = 0;
	for (int i = 0;; i++) {
		const int ch = cigar[i];
		if (!ch) break;
		if (ch >= '0' && ch <= '9') {
			if (tmpi < 0) tmpi = 0;
			tmpi = tmpi * 10 + (ch - '0');
		} else {
			if (tmpi < 0) tmpi = 1;
			if (old != ch && repeat > 0) {
				if (old == 'M' || old == 'S' || old == 'I') rlen += repeat;
				w += snprintf(out + w, 11, "%d%c", repeat, old);
				repeat = 0;
			}
			repeat += tmpi;
			tmpi = -1;
			old = ch;
		}
	}
	if (repeat > 0) {
		snprintf(out + w, 11, "%d%c", repeat, old);
		if (old == 'M' || old == 'S' || old == 'I') rlen += repeat;
	}
	return rlen;
}

static int plane_bit(const actx_t *c, int plane, unsigned int pos)
{
	if (!c->planes || pos >= c->plane_bits) return 0;
	return (c->planes[(uint64_t)plane * (c->plane_bits / 8) + pos / 8] >> (pos % 8)) & 1;
}

static int64_t weight_1sec(const actx_t *c, unsigned int pos, int len)
{
	int64_t ret = 10;
	for (unsigned int p = pos + 1; p <= pos + (unsigned int)len; p++) {
		if (plane_bit(c, 0, p)) return WEIGHT_TOP;
		if (plane_bit(c, 1, p)) ret = 13;
	}
	return ret;
}

static int64_t pos_weight(const actx_t *c, unsigned int pos, const char *cigar)
{
	int tmpi = 0, ch;
	int64_t best = 10;
	while ((ch = *cigar++) != 0) {
		if (ch >= '0' && ch <= '9') tmpi = tmpi * 10 + ch - '0';
		else {
			int add = 0;
			if (ch == 'M') {
				add = tmpi;
				const int64_t w = weight_1sec(c, pos, add);
				if (w > best) best = w;
				if (best >= WEIGHT_TOP) return best;
			} else if (ch == 'D' || ch == 'N' || ch == 'S') add = tmpi;
			pos += (unsigned int)add;
			tmpi = 0;
		}
	}
	return best;
}

typedef struct {
	int64_t score;
	uint32_t position;
	int flags, mapq, ed;
	int zero_mm, zero_rlen;    /* scored 0 for its mismatches / for rebuilt_rlen != read_len */
	int64_t weight;
	char cigar[MAXLEN * 4];
} cand_t;

static void explain(actx_t *c, const char *read_bin, int read_len, int applied, const slot_t *sl, cand_t *out)
{
	int16_t ind[TOLERANCE * 3 + 4];
	memset(ind, 0, sizeof ind);
	int move = 0, in_cigar = 0, mism = 0, matched = 0, mapped = 0, all_indel = 0;
	char piece[64], raw[MAXLEN * 8];
	const int neg = (sl->mask & NEGATIVE) != 0;
	const char *bin = read_bin + (neg ? REV_OFFSET : 0);
	unsigned int abs_pos = sl->pos;
	const int tolimax = sl->toli;
	recorder_copy(c, ind, sl->indel_recorder, tolimax, applied, &move);
	abs_pos += (unsigned int)move;
	int last_indel = ind[2], last_sub = ind[1] - 1, head = -1, last_mapped = 0;
	raw[0] = 0;
	for (int t = 3; t < tolimax; t += 3) {
		if (ind[t] == 0) break;
		const int v_first = ind[t] - 1, v_last = ind[t + 1] - 1, off = ind[t + 2], diff = off - last_indel;
		if (abs(diff) >= c->p.max_indel_length) continue;
		int lcb = subread_end(read_len, applied, last_sub) - 8;
		const int fcb = subread_end(read_len, applied, v_first) - 16 + 8;
		if (lcb < in_cigar) lcb = in_cigar;
		unsigned int meet = abs_pos + (unsigned int)lcb + (unsigned int)last_indel;
		if (head < 0) {
			const int fm = subread_end(read_len, applied, ind[0] - 1);
			head = soft_clipping(c, bin, 0, abs_pos, fm, 0, fm);
			if (head > 0) snprintf(raw, 11, "%dS", head);
			if (meet < (unsigned int)head + abs_pos) meet = (unsigned int)head + abs_pos;
			if (head > lcb) lcb = head;
			in_cigar = head;
		}
		int gap_mm = 0;
		int ipos = meet_in_the_middle(c, meet, bin, lcb, fcb - lcb, diff, &gap_mm);
		if (ipos == INVALID_INDEL) { ipos = (fcb - lcb) / 2; all_indel += abs(diff); }
		const int sec = match_bin(c, bin, in_cigar, abs_pos + (unsigned int)in_cigar + (unsigned int)last_indel, lcb - in_cigar);
		mism += gap_mm + (lcb - in_cigar - sec);
		matched += sec + fcb - lcb - gap_mm + (diff < 0 ? diff : 0);
		snprintf(piece, 45, "%dM%dM%d%c%dM", lcb - in_cigar, ipos, abs(diff), diff > 0 ? 'D' : 'I',
		         fcb - lcb - ipos + (diff < 0 ? diff : 0));
		mapped += fcb - in_cigar + (diff < 0 ? diff : 0);
		strcat(raw, piece);
		in_cigar = fcb;
		last_mapped = subread_end(read_len, applied, v_last) - 16 + 9;
		last_indel = off;
		last_sub = v_last;
	}
	if (head < 0) {
		const int fm = subread_end(read_len, applied, ind[0] - 1) - 8;
		head = soft_clipping(c, bin, 0, abs_pos, fm, 0, fm);
		if (head > 0) snprintf(raw, 11, "%dS", head);
		in_cigar = head;
		last_mapped = subread_end(read_len, applied, last_sub) - 16 + 8;
	}
	const int tail = soft_clipping(c, bin, last_mapped, abs_pos + (unsigned int)last_mapped + (unsigned int)last_indel,
	                               read_len - last_mapped, 1, 1);
	const int sec = match_bin(c, bin, in_cigar, abs_pos + (unsigned int)in_cigar + (unsigned int)last_indel,
	                          read_len - in_cigar - tail);
	mism += read_len - in_cigar - tail - sec;
	matched += sec;
	snprintf(piece, 11, "%dM", read_len - in_cigar - tail);
	mapped += read_len - in_cigar - tail;
	strcat(raw, piece);
	if (tail) { snprintf(piece, 11, "%dS", tail); strcat(raw, piece); }
	const int rebuilt = reduce_cigar(raw, out->cigar);
	const int64_t weight = pos_weight(c, abs_pos, out->cigar);
	int64_t score = 0;
	if (rebuilt == read_len && mapped >= c->p.min_mapped_length_for_mapped_read)
		score = (mism > c->p.max_mismatching_bases_in_reads ? 0 : (int64_t)((uint64_t)matched * 1000000llu / (1llu + (uint64_t)mism))) * weight;
	out->score = score;
	out->zero_rlen = rebuilt != read_len;
	out->zero_mm = rebuilt == read_len && mapped >= c->p.min_mapped_length_for_mapped_read && mism > c->p.max_mismatching_bases_in_reads;
	out->weight = weight;
	out->position = abs_pos;
	out->flags = neg ? 16 : 0;
	out->mapq = 40 - mism;
	out->ed = mism + all_indel;
}

static void top_three(int *top, int v)
{
	if (v <= top[2]) return;
	for (int x = 0; x < 3; x++) {
		if (v > top[x]) {
			for (int y = 2; y > x; y--) top[y] = top[y - 1];
			top[x] = v;
			break;
		} else if (v == top[x]) break;
	}
}

static void sort_scores(int *ix, const cand_t *cd, int low, int high)
{
	int i = low - 1;
	for (int j = low; j < high; j++) {
		const int64_t a = cd[ix[j]].score, b = cd[ix[high]].score;
		if ((a > b ? -1 : a < b ? 1 : 0) <= 0) {
			i++;
			const int t = ix[i]; ix[i] = ix[j]; ix[j] = t;
		}
	}
	{ const int t = ix[i + 1]; ix[i + 1] = ix[high]; ix[high] = t; }
	if (i > low) sort_scores(ix, cd, low, i);
	if (high > i + 2) sort_scores(ix, cd, i + 2, high);
}

/* read_bin of cellCounts_do_voting (:3084-3106): base2int codes, LSB first, four per byte */
static void build_read_bin(char *bin, const char *text, int len)
{
	char rev[MAXLEN + 1];
	reverse_complement(rev, text, len);
	memset(bin, 0, REV_OFFSET * 2);
	for (int s = 0; s < 2; s++)
		for (int i = 0; i < len; i++) bin[s * REV_OFFSET + i / 4] |= (char)(base2int((s ? rev : text)[i]) << (i % 4 * 2));
}

/* one read -> its head and up to max_reported records at out; returns the record count, or -1
 * where a record's CIGAR does not fit the field */
static int align_read(actx_t *c, const index_t *ix, const char *text, int len, ahead_t *h, aln_t *out)
{
	head_t vh;
	slot_t vs[ROWS * SPACE];
	memset(h, 0, sizeof *h);
	vote_read(ix, text, len, c->p.total_subreads, c->p.max_indel_length, &vh, vs);
	/* applied_subreads 1: find_subread_end divides by zero in the reference; no candidates here */
	if (vh.applied_subreads < 2) return 0;
	char bin[REV_OFFSET * 2];
	build_read_bin(bin, text, len);
	cand_t cd[MAX_REPORT];
	int count = 0, multi = 0;
	if (vh.max_vote >= c->p.min_votes_per_mapped_read) {
		int top[3] = {0, 0, 0};
		for (int k = 0; k < vh.n_slots; k++)
			if (vs[k].votes >= c->p.min_votes_per_mapped_read) top_three(top, vs[k].votes);
		for (int d = 0; d < 3 && count < c->max_voting_simples; d++) {
			const int N = top[d];
			if (N < 1 || top[0] - N > c->p.max_differential_from_top_vote_number) break;
			for (int k = 0; k < vh.n_slots && count < c->max_voting_simples; k++)   /* (compact order = row-major) */
				if (vs[k].votes == N) {
					explain(c, bin, len, vh.applied_subreads, &vs[k], &cd[count]);
					if (cd[count].score > 0) multi++;
					count++;
				}
		}
		if (multi > c->p.max_reported_alignments_per_read) multi = c->p.max_reported_alignments_per_read;
	}
	for (int i = 0; i < count; i++) {
		if (cd[i].zero_mm) c->edges |= EDGE_ZERO_MM;
		if (cd[i].zero_rlen) c->edges |= EDGE_ZERO_RLEN;
		if (cd[i].score > 0 && cd[i].weight == 13) c->edges |= EDGE_W13;
		if (cd[i].score > 0 && cd[i].weight == WEIGHT_TOP) c->edges |= EDGE_WTOP;
	}
	{
		int64_t best = 0;
		int at = 0;
		for (int i = 0; i < count; i++)
			if (cd[i].score > best) { best = cd[i].score; at = 1; }
			else if (cd[i].score == best && best > 0) at++;
		if (at > 1) c->edges |= EDGE_TIE;
	}
	h->multi_alignment_no = (uint16_t)multi;
	if (!multi) return 0;
	int order[MAX_REPORT], n = 0;
	for (int i = 0; i < count; i++) order[i] = i;
	sort_scores(order, cd, 0, count - 1);
	for (int a = 0; a < multi; a++) {
		const cand_t *k = &cd[order[a]];
		if (k->score < 1) continue;
		if (a >= c->p.max_reported_alignments_per_read) break;
		if (strlen(k->cigar) >= CIGAR_FIELD) return -1;
		aln_t *r = &out[n++];
		memset(r, 0, sizeof *r);
		r->score = k->score;
		r->position = k->position;
		r->flags = (int16_t)k->flags;
		r->mapq = (int16_t)k->mapq;
		r->editing_distance = k->ed;
		strcpy(r->cigar, k->cigar);
	}
	h->n_records = (uint16_t)n;
	return n;
}

/* svg_cell_set_exons's planes (:938-959): exon bases, and exon bases with 100 bases of flank */
void cellalign_model_planes(const uint32_t *starts, const uint32_t *stops, uint64_t n, uint8_t *planes, uint64_t plane_bits)
{
	memset(planes, 0, (size_t)(plane_bits / 8) * 2);
	for (uint64_t e = 0; e < n; e++) {
		const unsigned int a = starts[e], b = stops[e];
		if (a > 0xffffff00u || b > 0xffffff00u) continue;
		for (unsigned int p = a; p <= b; p++)
			if (p < plane_bits) planes[p / 8] |= (uint8_t)(1 << (p % 8));
		for (unsigned int p = a - 100; p <= b + 100; p++)
			if (p < plane_bits) planes[plane_bits / 8 + p / 8] |= (uint8_t)(1 << (p % 8));
	}
}

int cellalign_params_ok(const aparams_t *p)
{
	return p->total_subreads >= 7 && p->total_subreads <= 20 && p->max_indel_length == 5 && p->min_votes_per_mapped_read >= 1 &&
	       p->min_votes_per_mapped_read <= 64 && p->max_differential_from_top_vote_number >= 1 &&
	       p->max_differential_from_top_vote_number <= 30 && p->max_mismatching_bases_in_reads >= 0 &&
	       p->max_mismatching_bases_in_reads <= 100 && p->min_mapped_length_for_mapped_read >= -1 &&
	       p->min_mapped_length_for_mapped_read <= MAXLEN && p->max_reported_alignments_per_read >= 1 &&
	       p->max_reported_alignments_per_read <= MAX_REPORT;
}

/* heads[n]; alns: room for n * max_reported records, filled compactly; outside[n] (or NULL): per
 * read, the genome bases its candidates asked outside the image plus the recorder overruns;
 * edges[n] (or NULL): per read, its EDGE_* bits.
 * Returns the record count, -1 for refused arguments; aborts where a CIGAR overflows its field. */
int64_t cellalign_model(uint32_t nb, int gap, const uint32_t *bstart, const int16_t *keys, const uint32_t *vals,
                        const uint8_t *values, uint32_t values_bytes, uint32_t start_base_offset, const uint8_t *planes,
                        uint64_t plane_bits, const char *seq, const uint64_t *off, const uint16_t *len, uint64_t n,
                        const aparams_t *p, ahead_t *heads, aln_t *alns, uint32_t *outside, uint32_t *edges)
{
	if (!cellalign_params_ok(p)) return -1;
	for (uint64_t r = 0; r < n; r++)
		if (len[r] > MAXLEN) return -1;
	index_t ix = {nb, gap, bstart, keys, vals};
	actx_t c;
	memset(&c, 0, sizeof c);
	c.values = values; c.values_bytes = values_bytes; c.start_base_offset = start_base_offset;
	c.planes = planes; c.plane_bits = plane_bits;
	c.p = *p;
	c.max_voting_simples = p->max_reported_alignments_per_read > 3 ? p->max_reported_alignments_per_read : 3;   /* :518, :604 */
	uint64_t k = 0;
	for (uint64_t r = 0; r < n; r++) {
		c.outside = c.overrun = 0;
		c.edges = 0;
		const int got = align_read(&c, &ix, seq + off[r], len[r], &heads[r], alns + k);
		if (got < 0) { fprintf(stderr, "cellalign_model: read %llu: a CIGAR longer than its field\n", (unsigned long long)r); abort(); }
		if (got) heads[r].first_record = k;
		k += (uint64_t)got;
		if (outside) outside[r] = (uint32_t)(c.outside + c.overrun);
		if (edges) edges[r] = c.edges;
	}
	return (int64_t)k;
}
