/* TEST INFRASTRUCTURE ONLY: a plain-C restatement of cellCounts' UMI stage on the structs of
 * include/subread_vote.h, against which the GPU path (subread_amd/csrc/svg_cell_count.hip) is
 * compared.  No part of the library is built from this file.  The four stages, as read from
 * cell-counts.c:
 *   support count   ADD_key_struct (:3945-3949) and cellCounts_do_one_batch_tab_to_struct_list (:3756-3775)
 *   step 1          the comparator of :3725-3754 with sort_by_geneid_then_umi, the sections of
 *                   cellCounts_do_one_batch_UMI_merge_one_step (:3644-3678) and the two rules of
 *                   cellCounts_do_one_batch_UMI_merge_one_cell (:3552-3641)
 *   step 2          the same comparator without the flag, and :3528-3538, :3672
 *   count table     ADD_count_hash (:3520)
 * Text UMIs and qsort throughout: nothing of the device code's packed keys is used here. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "subread_vote.h"

typedef struct { int32_t sample, cell; int64_t gene; char umi[SVG_CELL_MAX_UMI]; } umi_obs;

static int g_len;   /* the UMI length of the run (qsort takes no context) */

static int obs_cmp(const void *a, const void *b)
{
	const umi_obs *l = a, *r = b;
	if (l->sample != r->sample) return l->sample < r->sample ? -1 : 1;
	if (l->cell != r->cell) return l->cell < r->cell ? -1 : 1;
	if (l->gene != r->gene) return l->gene < r->gene ? -1 : 1;
	return memcmp(l->umi, r->umi, (size_t)g_len);
}

/* :3725-3754 with sort_by_geneid_then_umi = 1, the samples being lists of their own (:3774) */
static int step1_cmp(const void *a, const void *b)
{
	const svg_cell_umi_entry *l = a, *r = b;
	if (l->sample != r->sample) return l->sample < r->sample ? -1 : 1;
	if (l->cell != r->cell) return l->cell < r->cell ? -1 : 1;
	if (l->gene != r->gene) return l->gene < r->gene ? -1 : 1;
	if (l->support != r->support) return l->support < r->support ? 1 : -1;
	return memcmp(l->umi, r->umi, (size_t)g_len);
}

static const svg_cell_umi_entry *g_entries;

/* the same with sort_by_geneid_then_umi = 0, over indexes of the survivors */
static int step2_cmp(const void *a, const void *b)
{
	const svg_cell_umi_entry *l = g_entries + *(const uint32_t *)a, *r = g_entries + *(const uint32_t *)b;
	if (l->sample != r->sample) return l->sample < r->sample ? -1 : 1;
	if (l->cell != r->cell) return l->cell < r->cell ? -1 : 1;
	const int u = memcmp(l->umi, r->umi, (size_t)g_len);
	if (u) return u;
	if (l->support_merged != r->support_merged) return l->support_merged < r->support_merged ? 1 : -1;
	if (l->gene != r->gene) return l->gene < r->gene ? -1 : 1;
	return 0;
}

/* cellCounts_hamming_max2_fixlen (:3511) */
static int hamming_max2(const char *a, const char *b, int len)
{
	int ret = 0;
	for (int x = 0; x < len; x++) {
		if (a[x] != b[x]) ret++;
		if (ret > 1) return ret;
	}
	return ret;
}

/* one (cell, gene) section [a, b) (:3552-3641).  rule 0: the reference's choice by size; 1: the
 * list rule; 2: the looktable rule.  acc holds the accepted entries in acceptance order */
static void step1_section(svg_cell_umi_entry *e, uint32_t a, uint32_t b, int L, int rule, uint32_t *acc)
{
	const int look = rule == 2 || (rule == 0 && b - a > 30);
	const int half = L / 2;
	uint32_t nacc = 0;
	for (uint32_t i = a; i < b; i++) {
		int found = 0;
		for (int hx = 0; hx < (look ? 2 : 1) && !found; hx++)
			for (uint32_t k = 0; k < nacc; k++) {
				svg_cell_umi_entry *q = e + acc[k];
				/* the list of key 'F' + umi[0 .. half) or 'S' + umi[half .. 2 half) holds the acceptors with that key, in acceptance order */
				if (look && memcmp(q->umi + hx * half, e[i].umi + hx * half, (size_t)half)) continue;
				if (hamming_max2(q->umi, e[i].umi, L) < 2) {
					found = 1;
					q->support_merged += e[i].support_merged;
					e[i].outcome = SVG_CELL_UMI_MERGED;
					memcpy(e[i].acceptor_umi, q->umi, (size_t)L);
					break;
				}
			}
		if (!found) acc[nacc++] = i;
	}
}

/* -> 0, or -1 for a value outside the contract (a UMI character, a sample above n_samples, a cell
 * of 2^24 or more, a gene outside 0..2^31-1), -2 out of memory.  entries and counts have room for
 * n records; removed for n_samples; dropped for 2 */
int cellumi_model(const int32_t *sample, const int32_t *cell, const int64_t *gene, const char *umi, uint64_t n, int L, int n_samples,
                  int rule, svg_cell_umi_entry *entries, uint64_t *n_entries, svg_cell_count *counts, uint64_t *n_counts,
                  uint64_t *removed, uint64_t *dropped)
{
	*n_entries = *n_counts = 0;
	dropped[0] = dropped[1] = 0;
	memset(removed, 0, 8 * (size_t)n_samples);
	if (L < 1 || L > SVG_CELL_MAX_UMI) return -1;
	g_len = L;
	umi_obs *o = malloc(sizeof *o * (n + 1));
	uint32_t *acc = malloc(4 * (n + 1)), *ord = malloc(4 * (n + 1));
	if (!o || !acc || !ord) { free(o); free(acc); free(ord); return -2; }
	uint64_t m = 0;
	for (uint64_t i = 0; i < n; i++) {
		for (int k = 0; k < L; k++)
			if (!strchr("ACGTN", umi[i * (uint64_t)L + k]) || !umi[i * (uint64_t)L + k]) { free(o); free(acc); free(ord); return -1; }
		if (sample[i] > n_samples || cell[i] >= SVG_CELL_MAX_CELLS || gene[i] < 0 || gene[i] > 0x7fffffffll) { free(o); free(acc); free(ord); return -1; }
		if (sample[i] <= 0) { dropped[0]++; continue; }
		if (cell[i] < 0) { dropped[1]++; continue; }     /* :3658: both steps skip it */
		memset(&o[m], 0, sizeof o[m]);
		o[m].sample = sample[i]; o[m].cell = cell[i]; o[m].gene = gene[i];
		memcpy(o[m].umi, umi + i * (uint64_t)L, (size_t)L);
		m++;
	}
	/* the support count */
	qsort(o, m, sizeof *o, obs_cmp);
	uint64_t ne = 0;
	for (uint64_t i = 0; i < m; i++) {
		if (i && !obs_cmp(&o[i], &o[i - 1])) { entries[ne - 1].support++; entries[ne - 1].support_merged++; continue; }
		svg_cell_umi_entry *q = entries + ne++;
		memset(q, 0, sizeof *q);
		q->sample = o[i].sample; q->cell = o[i].cell; q->gene = (int32_t)o[i].gene;
		q->support = q->support_merged = 1;
		q->outcome = SVG_CELL_UMI_LOST;
		memcpy(q->umi, o[i].umi, (size_t)L);
	}
	/* step 1 */
	qsort(entries, ne, sizeof *entries, step1_cmp);
	for (uint64_t a = 0, i = 1; i <= ne; i++)
		if (i == ne || entries[i].sample != entries[a].sample || entries[i].cell != entries[a].cell || entries[i].gene != entries[a].gene) {
			if (i - a > 1) step1_section(entries, (uint32_t)a, (uint32_t)i, L, rule, acc);
			a = i;
		}
	/* step 2 */
	uint64_t n2 = 0;
	for (uint64_t i = 0; i < ne; i++)
		if (entries[i].outcome != SVG_CELL_UMI_MERGED) ord[n2++] = (uint32_t)i;
	g_entries = entries;
	qsort(ord, n2, 4, step2_cmp);
	for (uint64_t a = 0, i = 1; i <= n2; i++) {
		const svg_cell_umi_entry *x = entries + ord[a], *y = i < n2 ? entries + ord[i] : NULL;
		if (y && y->sample == x->sample && y->cell == x->cell && !memcmp(y->umi, x->umi, (size_t)L)) continue;
		svg_cell_umi_entry *first = entries + ord[a];
		if (i - a == 1 || first->support_merged > entries[ord[a + 1]].support_merged) first->outcome = SVG_CELL_UMI_COUNTED;
		else { first->outcome = SVG_CELL_UMI_REMOVED; removed[first->sample - 1]++; }
		a = i;
	}
	/* the count table: the entries stand by (sample, cell, gene) */
	uint64_t nc = 0;
	for (uint64_t i = 0; i < ne; i++) {
		if (entries[i].outcome != SVG_CELL_UMI_COUNTED) continue;
		if (nc && counts[nc - 1].sample == entries[i].sample && counts[nc - 1].cell == entries[i].cell && counts[nc - 1].gene == entries[i].gene) {
			counts[nc - 1].n_umis++;
			continue;
		}
		counts[nc].sample = entries[i].sample; counts[nc].cell = entries[i].cell; counts[nc].gene = entries[i].gene;
		counts[nc].n_umis = 1;
		nc++;
	}
	*n_entries = ne;
	*n_counts = nc;
	free(o); free(acc); free(ord);
	return 0;
}

/* the UMI code that ships (subread_amd/csrc/svg_cell_umi.h, which svg_cell_count.hip includes), exported
 * for the CPU tests of the two properties the kernels rest on; the model above does not use it */
#include "../../subread_amd/csrc/svg_cell_umi.h"

uint64_t cellumi_code(const char *umi, int L) { return umi_encode(umi, L); }
int cellumi_code_hamming(uint64_t a, uint64_t b) { return umi_hamming(a, b); }
uint64_t cellumi_half_mask(int L, int second) { return umi_half_mask(L, second); }
uint32_t cellumi_packed_code(uint32_t base, uint32_t exception) { return umi_packed_code(base, exception); }
void cellumi_decode(uint64_t code, int L, char *out) { umi_decode(code, L, out); }

int cellumi_hamming_max2(const char *a, const char *b, int L) { return hamming_max2(a, b, L); }
