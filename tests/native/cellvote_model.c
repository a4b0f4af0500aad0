/* TEST INFRASTRUCTURE ONLY: cellCounts' voting step of one read, restated in plain C over the
 * flat index arrays (bucket starts, i16 keys, u32 positions), in svg_cell_vote_batch's record
 * format (include/subread_vote.h).  Reference lines (Subread v2.0.6):
 *   cellCounts_do_voting                    cell-counts.c:3051-3131  (plan and intake, :3077-3101)
 *   prefill_votes                           cell-counts.c:432-489
 *   cellCounts_process_copy_ptrs_to_votes   cell-counts.c:2786-2881
 *   quick_sort_run                          core.c:4694-4714
 *   reverse_read                            input-files.c:1111-1160
 * Reads are ASCII here (the library takes them 2-bit packed), so the packed key path is checked
 * against an independent one.  Built as a shared object by tests/cellvote_common.py. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>

#define ROWS 17            /* GENE_SCRNA_VOTE_TABLE_SIZE, cell-counts.c:34 */
#define SPACE 3            /* GENE_SCRNA_VOTE_SPACE, cell-counts.c:33 */
#define RECORDER 21        /* MAX_INDEL_TOLERANCE * 3, subread.h:225 */
#define NEGATIVE 2048      /* IS_NEGATIVE_STRAND, subread.h:107 */
#define PRIME 66889        /* VOTING_PRIME_NUMBER, cell-counts.c:2749 */
#define MAXLEN 160         /* MAX_SCRNA_READ_LENGTH, subread.h:502 */

typedef struct {           /* svg_cell_head */
	uint64_t first_slot;
	uint16_t n_slots;
	int16_t max_vote;
	int16_t applied_subreads;
	uint8_t items[ROWS];
	uint8_t pad;
} head_t;

typedef struct {           /* svg_cell_slot */
	uint32_t pos;
	int16_t mask;
	int16_t votes;
	int16_t coverage_start, coverage_end;
	uint8_t toli;
	uint8_t pad;
	int16_t indel_recorder[RECORDER];
} slot_t;

typedef struct {
	uint32_t nb;
	int gap;
	const uint32_t *bstart;
	const int16_t *keys;
	const uint32_t *vals;
} index_t;

static int base2int(int c) { return c < 'G' ? (c == 'A' ? 0 : 2) : (c == 'G' ? 1 : 3); }   /* subread.h:238 */

/* reverse_read for base space: A<->T, C<->G, anything else becomes 'N' */
static void reverse_complement(char *dst, const char *src, int len)
{
	for (int i = 0; i < len; i++) {
		const char c = src[len - 1 - i];
		dst[i] = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'U' ? 'A' : 'N';
	}
}

/* prefill_votes: the equal-key run of `subread` in its bucket -> first item (global), length */
static void prefill(const index_t *ix, uint32_t subread, uint32_t *first, int *count)
{
	const uint32_t b = subread % ix->nb, base = ix->bstart[b];
	const int items = (int)(ix->bstart[b + 1] - base);
	const int16_t *ck = ix->keys + base;
	*first = 0;
	*count = 0;
	if (!items) return;
	int imin = 0, imax = items - 1, last;
	const short key = (short)(subread / ix->nb);
	for (;;) {
		last = (imin + imax) / 2;
		const short cur = ck[last];
		if (cur > key) imax = last - 1;
		else if (cur < key) imin = last + 1;
		else break;
		if (imax < imin) return;
	}
	imax -= imin;
	const int start = last;
	int stoploc, tl;
	for (int step = imax / 4; step > 1; step /= 3)
		for (;;) {
			tl = last + step;
			if (tl >= items || ck[tl] != key) break;
			last = tl;
		}
	for (;;) {
		last++;
		if (last == items || ck[last] != key) { stoploc = last; last = start; break; }
	}
	for (int step = imax / 4; step > 1; step /= 3)
		for (;;) {
			tl = last - step;
			if (tl < imin || ck[tl] != key) break;
			last = tl;
		}
	while (!(last == imin || ck[last - 1] != key)) last--;
	*first = base + (uint32_t)last;
	*count = stoploc - last;
}

/* quick_sort_run with cellCounts' compare (difference of run lengths) and exchange */
static void sort_run(int *no, const int *votes, int low, int high)
{
	const int pivot = high;
	int i = low - 1;
	for (int j = low; j < high; j++)
		if (votes[no[j]] - votes[no[pivot]] <= 0) {
			i++;
			const int t = no[i]; no[i] = no[j]; no[j] = t;
		}
	{ const int t = no[i + 1]; no[i + 1] = no[high]; no[high] = t; }
	if (i > low) sort_run(no, votes, low, i);
	if (high > i + 2) sort_run(no, votes, i + 2, high);
}

#define ROW_OF(k) (((unsigned int)(k) / 5) % ROWS)   /* _index_vote_tol, cell-counts.c:2752 */

/* one read: head h, slots appended at out (room for ROWS * SPACE); returns the slot count */
static int vote_read(const index_t *ix, const char *text, int len, int total_subreads, int max_indel, head_t *h, slot_t *out)
{
	memset(h, 0, sizeof *h);
	if (len < 16) return 0;                                            /* :3077 */
	const int cr = (int)((unsigned)(len - 15 - ix->gap) << 16);        /* :3079 (arithmetic shift of the reference) */
	int step = cr / (total_subreads - 1);
	if (step < (ix->gap << 16)) step = ix->gap << 16;
	const int applied = 1 + cr / step;
	char rev[MAXLEN + 1];
	reverse_complement(rev, text, len);
	int votes[40], offsets[40];
	uint32_t first[40];
	for (int s = 0; s < 2; s++)
		for (int k = 0; k < applied; k++) {
			const int off = (int)(((int64_t)step * k) >> 16);
			const char *t = (s ? rev : text) + off;
			uint32_t key = 0;
			for (int i = 0; i < 16; i++) key = (key << 2) | (uint32_t)base2int(t[i]);
			prefill(ix, key, &first[s * applied + k], &votes[s * applied + k]);
			offsets[s * applied + k] = off;
		}
	const int subreads = 2 * applied;
	int no[40];
	for (int i = 0; i < subreads; i++) no[i] = i;
	sort_run(no, votes, 0, subreads - 1);

	uint32_t pos[ROWS][SPACE];
	slot_t tab[ROWS][SPACE];
	int items[ROWS];
	memset(items, 0, sizeof items);
	int max_vote = 0;
	for (int x1 = 0; x1 < subreads; x1++) {
		const int myno = no[x1], has = votes[myno];
		if (has < 1) continue;
		const int p1 = myno % applied + 1, offset = offsets[myno], of16 = offset + 16;
		const int mask = myno >= applied ? NEGATIVE : 0;
		int sum = votes[no[subreads - 1]];
		for (int x2 = 0; x2 < has; x2++) {
			const unsigned int kv = ix->vals[first[myno] + (uint32_t)(sum % has)] - (unsigned)offset;
			sum += PRIME;
			const int home = (int)ROW_OF(kv), homelen = items[home];
			int found = 0;
			for (int iix = 0; iix <= 5 && !found; iix = iix > 0 ? -iix : -iix + 5) {
				const int row = iix ? (int)ROW_OF(kv + iix) : home;
				for (int it = 0; it < items[row]; it++) {
					const int dist = (int)(kv - pos[row][it]);
					slot_t *sl = &tab[row][it];
					if (dist < -max_indel || dist > max_indel || sl->mask != mask) continue;
					int known = 0;
					for (int t = 0; t < sl->toli; t += 3)
						if (sl->indel_recorder[t + 2] == dist) {
							if (sl->indel_recorder[t] > p1) sl->indel_recorder[t] = (int16_t)p1;
							if (sl->indel_recorder[t + 1] < p1) sl->indel_recorder[t + 1] = (int16_t)p1;
							known = 1;
							break;
						}
					if (sl->toli < RECORDER && !known) {
						sl->indel_recorder[sl->toli] = (int16_t)p1;
						sl->indel_recorder[sl->toli + 1] = (int16_t)p1;
						sl->indel_recorder[sl->toli + 2] = (int16_t)dist;
						sl->toli += 3;
					}
					sl->votes++;
					if (max_vote < sl->votes) max_vote = sl->votes;
					if (offset < sl->coverage_start) sl->coverage_start = (int16_t)offset;
					if (of16 > sl->coverage_end) sl->coverage_end = (int16_t)of16;
					found = 1;
					break;
				}
			}
			if (!found && homelen < SPACE) {
				slot_t *sl = &tab[home][homelen];
				memset(sl, 0, sizeof *sl);
				items[home] = homelen + 1;
				pos[home][homelen] = kv;
				sl->pos = kv;
				sl->mask = (int16_t)mask;
				sl->votes = 1;
				sl->indel_recorder[0] = sl->indel_recorder[1] = (int16_t)p1;
				sl->toli = 3;
				sl->coverage_start = (int16_t)offset;
				sl->coverage_end = (int16_t)of16;
				if (max_vote == 0) max_vote = 1;
			}
		}
	}
	int n = 0;
	for (int r = 0; r < ROWS; r++) {
		h->items[r] = (uint8_t)items[r];
		for (int it = 0; it < items[r]; it++) out[n++] = tab[r][it];
	}
	h->n_slots = (uint16_t)n;
	h->max_vote = (int16_t)max_vote;
	h->applied_subreads = (int16_t)applied;
	return n;
}

typedef struct {
	index_t ix;
	const char *seq;
	const uint64_t *off;
	const uint16_t *len;
	uint64_t lo, hi;
	int total_subreads, max_indel;
	head_t *heads;
	slot_t *staging;     /* ROWS * SPACE records per read */
} job_t;

static void *worker(void *p)
{
	job_t *j = (job_t *)p;
	for (uint64_t r = j->lo; r < j->hi; r++)
		vote_read(&j->ix, j->seq + j->off[r], j->len[r], j->total_subreads, j->max_indel, &j->heads[r],
		          j->staging + r * ROWS * SPACE);
	return NULL;
}

/* heads[n]; slots: room for n * 51 records, compacted in place; returns the slot count, or -1 for
 * a bad argument (the refusals of svg_cell_vote_batch) */
int64_t cellvote_model(uint32_t nb, int gap, const uint32_t *bstart, const int16_t *keys, const uint32_t *vals,
                       const char *seq, const uint64_t *off, const uint16_t *len, uint64_t n, int total_subreads,
                       int max_indel, int threads, head_t *heads, slot_t *slots)
{
	if (total_subreads < 7 || total_subreads > 20 || max_indel != 5) return -1;
	for (uint64_t r = 0; r < n; r++)
		if (len[r] > MAXLEN) return -1;
	if (threads < 1) threads = 1;
	if (threads > 64) threads = 64;
	pthread_t th[64];
	job_t jobs[64];
	for (int t = 0; t < threads; t++) {
		job_t *j = &jobs[t];
		j->ix.nb = nb; j->ix.gap = gap; j->ix.bstart = bstart; j->ix.keys = keys; j->ix.vals = vals;
		j->seq = seq; j->off = off; j->len = len;
		j->lo = n * (uint64_t)t / (uint64_t)threads;
		j->hi = n * (uint64_t)(t + 1) / (uint64_t)threads;
		j->total_subreads = total_subreads; j->max_indel = max_indel;
		j->heads = heads; j->staging = slots;
		pthread_create(&th[t], NULL, worker, j);
	}
	for (int t = 0; t < threads; t++) pthread_join(th[t], NULL);
	uint64_t k = 0;
	for (uint64_t r = 0; r < n; r++) {
		if (heads[r].applied_subreads) heads[r].first_slot = k;   /* (a skipped read keeps its zero head) */
		if (k != r * ROWS * SPACE) memmove(slots + k, slots + r * ROWS * SPACE, sizeof(slot_t) * heads[r].n_slots);
		k += heads[r].n_slots;
	}
	return (int64_t)k;
}
