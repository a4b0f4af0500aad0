/* TEST INFRASTRUCTURE ONLY: a plain-C model of what svg_cell_assign_batch adds to
 * svg_cell_align_batch, written at the level of the reference's loops over the tables of the host
 * builder (subread_amd/csrc/svg_cell_annot.c, linked beside this file):
 *   cellCounts_write_read_in_batch_bin          cell-counts.c:2061-2088
 *   locate_gene_position_max (rl = 0)           gene-algorithms.c:441-511
 *   get_soft_clipping_length                    core.c:1232-1247
 *   cellCounts_find_hits_for_mapped_section     cell-counts.c:1575-1654
 *   cellCounts_summarize_entrez_hits            :2039-2059, and the rule of :1982
 *   cellCounts_get_cellbarcode_no               :1701-1768, hamming_dist_ATGC_max2 input-blc.c:1109-1120
 * Unlike the kernel it keeps the raw hit list of an alignment and summarises it afterwards, as the
 * reference does, and it compares barcodes as text. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../subread_amd/csrc/svg_cell_annot.h"

#define BUCKET 131072

typedef struct { int64_t *v; int64_t n, cap; } list_t;

static void push(list_t *l, int64_t x)
{
	if (l->n == l->cap) { l->cap = l->cap ? l->cap * 2 : 16; l->v = realloc(l->v, sizeof(int64_t) * (size_t)l->cap); }
	l->v[l->n++] = x;
}

static void find_hits(const svg_cell_annot *a, uint32_t c, int section_begin_pos, int section_end_pos, int is_negative, list_t *hits)
{
	int start_index = section_begin_pos / BUCKET, end_index = (1 + section_end_pos) / BUCKET;
	const int top = (int)(a->chro_len[c] / BUCKET);
	if (start_index > top) start_index = top;
	if (end_index > top + 1) end_index = top + 1;
	const uint32_t *rt = a->rev + a->rev_first[c];
	unsigned int search_start = 0xffffffffu;
	while (start_index <= end_index) {
		search_start = rt[start_index];
		if (search_start < 0xffffff00) break;
		start_index++;
	}
	if (search_start > 0xffffff00) return;
	for (unsigned int block = search_start; block < a->chro_block_end[c]; block++) {
		if ((int64_t)a->block_min[block] > section_end_pos) break;
		if ((int64_t)a->block_max[block] < section_begin_pos) continue;
		int item = block > 0 ? (int)a->block_end[block - 1] : 0;
		const int item_end = (int)a->block_end[block];
		for (; item < item_end; item++)
			if ((int64_t)a->end[item] >= section_begin_pos) {
				if ((int64_t)a->start[item] > section_end_pos) break;
				if (is_negative == a->strand[item]) push(hits, item);
			}
	}
}

/* -> contig or -1, *pos */
static int locate(const uint32_t *chr_end, uint32_t n_chr, int padding, uint32_t linear, int *pos)
{
	int low = 0, high = (int)n_chr, n;
	*pos = -1;
	while (1) {
		if (high <= low + 1) { n = low - 2 > 0 ? low - 2 : 0; break; }
		const int mid = (low + high) / 2;
		if (chr_end[mid] > linear) high = mid; else low = mid + 1;
	}
	for (; n < (int)n_chr; n++)
		if (chr_end[n] > linear) {
			*pos = n == 0 ? (int)linear : (int)(linear - chr_end[n - 1]);
			if (0 + linear > chr_end[n] + 15 - (uint32_t)padding) return -1;
			if (*pos < padding) return -1;
			*pos -= padding;
			return n;
		}
	return -1;
}

static int soft_clip(const char *cigar)
{
	int v = 0;
	for (int i = 0; cigar[i] > 0; i++) {
		if (cigar[i] >= '0' && cigar[i] <= '9') v = v * 10 + (cigar[i] - '0');
		else return cigar[i] == 'S' ? v : 0;
	}
	return 0;
}

/* a: NULL = no annotation.  advance != 0: the cursor advances over M, D and N (what :2073-2083
 * compute and never apply) -- for the tests' "a fixed cursor would differ" class only.
 * -> genes written, or -1 when they do not fit cap */
int64_t cellassign_model(const svg_cell_annot *a, int allow_multi, int advance, const uint32_t *chr_end, uint32_t n_chr, int padding,
                         const svg_cell_aln *alns, uint64_t n, svg_cell_hit *hits, int32_t *genes, uint64_t cap)
{
	list_t raw = {NULL, 0, 0};
	uint64_t ng = 0;
	for (uint64_t i = 0; i < n; i++) {
		svg_cell_hit *h = hits + i;
		memset(h, 0, sizeof *h);
		char cigar[SVG_CELL_CIGAR + 1];
		memcpy(cigar, alns[i].cigar, SVG_CELL_CIGAR);
		cigar[SVG_CELL_CIGAR] = 0;
		int chro_pos = 0;
		h->contig = locate(chr_end, n_chr, padding, alns[i].position + 1u, &chro_pos);
		if (h->contig < 0) continue;
		chro_pos += soft_clip(cigar);
		h->chro_pos = chro_pos;
		if (!a) continue;
		const int is_negative = (alns[i].flags & 16) ? 1 : 0;
		int tmpi = 0, chro_curs = chro_pos;
		raw.n = 0;
		for (int k = 0; cigar[k]; k++) {
			const int nch = cigar[k];
			if (nch >= '0' && nch <= '9') tmpi = 10 * tmpi + (nch - '0');
			else {
				int add_curs = 0;
				if (nch == 'M' || nch == 'D' || nch == 'N') add_curs = tmpi;
				if (nch == 'M') find_hits(a, (uint32_t)h->contig, chro_curs, chro_curs + add_curs, is_negative, &raw);
				if (advance) chro_curs += add_curs;
				tmpi = 0;
			}
		}
		/* cellCounts_summarize_entrez_hits */
		int64_t nhits = raw.n, w = 0;
		for (int64_t s = 0; s < nhits; s++) raw.v[s] = a->gene[raw.v[s]];
		for (int64_t s = 0; s < nhits; s++) {
			int found = 0;
			for (int64_t k2 = 0; k2 < w; k2++) if (raw.v[k2] == raw.v[s]) found = 1;
			if (!found) raw.v[w++] = raw.v[s];
		}
		nhits = w;
		if (nhits > 1 && !allow_multi) nhits = 0;
		if (ng + (uint64_t)nhits > cap) { free(raw.v); return -1; }
		h->nhits = (uint32_t)nhits;
		if (nhits) h->first_gene = ng;
		for (int64_t s = 0; s < nhits; s++) genes[ng++] = (int32_t)raw.v[s];
	}
	free(raw.v);
	return (int64_t)ng;
}

/* the builder on a feature list, then the model: the form the Python tests call */
int64_t cellassign_model_features(const svg_cell_feature *f, uint64_t nf, int allow_multi, int advance, const uint32_t *chr_end, uint32_t n_chr,
                                  int padding, const svg_cell_aln *alns, uint64_t n, svg_cell_hit *hits, int32_t *genes, uint64_t cap)
{
	svg_cell_annot a;
	char why[256];
	if (!nf) return cellassign_model(NULL, allow_multi, advance, chr_end, n_chr, padding, alns, n, hits, genes, cap);
	if (svg_cell_annot_build(f, nf, chr_end, n_chr, padding, &a, why, sizeof why)) { fprintf(stderr, "cellassign_model: %s\n", why); return -2; }
	const int64_t r = cellassign_model(&a, allow_multi, advance, chr_end, n_chr, padding, alns, n, hits, genes, cap);
	svg_cell_annot_free(&a);
	return r;
}

/* the builder's tables as the fixture holds the reference's: counts[0] blocks, counts[1] reverse-table words;
 * contigs: chro_possible_length, chro_block_table_end and bins of each */
int cellassign_model_tables(const svg_cell_feature *f, uint64_t nf, const uint32_t *chr_end, uint32_t n_chr, int padding, uint32_t *start,
                            uint32_t *stop, uint8_t *strand, int32_t *gene, uint32_t *bend, uint32_t *bmin, uint32_t *bmax, uint32_t *contigs,
                            uint32_t *rev, uint32_t *counts)
{
	svg_cell_annot a;
	char why[256];
	if (svg_cell_annot_build(f, nf, chr_end, n_chr, padding, &a, why, sizeof why)) { fprintf(stderr, "cellassign_model: %s\n", why); return -2; }
	memcpy(start, a.start, 4 * (size_t)a.n_features); memcpy(stop, a.end, 4 * (size_t)a.n_features);
	memcpy(strand, a.strand, a.n_features); memcpy(gene, a.gene, 4 * (size_t)a.n_features);
	memcpy(bend, a.block_end, 4 * (size_t)a.n_blocks); memcpy(bmin, a.block_min, 4 * (size_t)a.n_blocks); memcpy(bmax, a.block_max, 4 * (size_t)a.n_blocks);
	for (uint32_t c = 0; c < n_chr; c++) {
		contigs[3 * c] = a.chro_len[c]; contigs[3 * c + 1] = a.chro_block_end[c]; contigs[3 * c + 2] = a.chro_len[c] / BUCKET + 2;
	}
	memcpy(rev, a.rev, 4 * (size_t)a.rev_words);
	counts[0] = a.n_blocks; counts[1] = a.rev_words;
	svg_cell_annot_free(&a);
	return 0;
}

static int is_ATGC(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; }

static int hamming_dist_ATGC_max2(const char *s1, const char *s2)
{
	int xx, ret = 0;
	for (xx = 0;; xx++) {
		if (is_ATGC(s1[xx]) && is_ATGC(s2[xx])) {
			ret += s1[xx] == s2[xx];
			if (xx - ret > 2) return 999;
		} else break;
	}
	return xx - ret;
}

/* the half key of cbc (which = 0: F, 1: S) as the builder's row number, or -1 where the text key
 * holds a character no whitelist key holds */
static int64_t half_row(const char *cbc, int L, int which)
{
	int64_t key = 0;
	for (int j = 0; j < L / 2; j++) {
		const char ch = cbc[2 * j + which];
		const int b = ch == 'A' ? 0 : ch == 'G' ? 1 : ch == 'C' ? 2 : ch == 'T' ? 3 : -1;
		if (b < 0) return -1;
		key |= (int64_t)b << (2 * j);
	}
	return key;
}

/* whitelist: n texts of L characters, each NUL-terminated (stride L + 1); cbc likewise */
int cellassign_model_barcode(const svg_cell_bcodes *b, const char *whitelist, const char *cbc)
{
	const int L = (int)b->length;
	list_t ret = {NULL, 0, 0};
	int tb1 = -1;
	for (int xx1 = 0; xx1 < 3; xx1++) {
		if (xx1 == 0) {
			/* the exact probe: the entry equal to cbc, if any, has cbc's F key */
			const int64_t row = half_row(cbc, L, 0);
			if (row < 0) continue;
			for (uint32_t q = b->frow[row]; q < b->frow[row + 1]; q++)
				if (!strncmp(whitelist + (size_t)b->fent[q] * (L + 1), cbc, (size_t)L)) { free(ret.v); return (int)b->fent[q]; }
		} else {
			const int64_t row = half_row(cbc, L, xx1 - 1);
			if (row < 0) continue;
			const uint32_t *rowp = xx1 == 1 ? b->frow : b->srow, *ent = xx1 == 1 ? b->fent : b->sent;
			for (uint32_t q = rowp[row]; q < rowp[row + 1]; q++) {
				int found = 0;
				for (int64_t k = 0; k < ret.n; k++) if (ret.v[k] == ent[q]) { found = 1; break; }
				if (!found) push(&ret, ent[q]);
			}
		}
	}
	for (int64_t k = 0; k < ret.n; k++)
		if (hamming_dist_ATGC_max2(whitelist + (size_t)ret.v[k] * (L + 1), cbc) == 1) { tb1 = (int)ret.v[k]; break; }
	free(ret.v);
	return tb1;
}

/* the same with the whitelist image built once and shared by several callers (threads over ranges of reads) */
void *cellassign_model_bcodes_new(const char *whitelist, uint64_t nwl, int L)
{
	svg_cell_bcodes *b = malloc(sizeof *b);
	char why[256];
	const char **ptr = malloc(sizeof(char *) * (nwl ? nwl : 1));
	for (uint64_t i = 0; i < nwl; i++) ptr[i] = whitelist + i * (size_t)(L + 1);
	const int rc = svg_cell_bcodes_build(ptr, nwl, L, b, why, sizeof why);
	free(ptr);
	if (rc) { fprintf(stderr, "cellassign_model: %s\n", why); free(b); return NULL; }
	return b;
}

void cellassign_model_bcodes_run(const void *h, const char *whitelist, const char *reads, uint64_t n, int32_t *out)
{
	const svg_cell_bcodes *b = h;
	for (uint64_t i = 0; i < n; i++) out[i] = cellassign_model_barcode(b, whitelist, reads + i * (size_t)(b->length + 1));
}

void cellassign_model_bcodes_free(void *h)
{
	svg_cell_bcodes_free(h);
	free(h);
}

void *cellassign_model_annot_new(const svg_cell_feature *f, uint64_t nf, const uint32_t *chr_end, uint32_t n_chr, int padding)
{
	svg_cell_annot *a = malloc(sizeof *a);
	char why[256];
	if (svg_cell_annot_build(f, nf, chr_end, n_chr, padding, a, why, sizeof why)) { fprintf(stderr, "cellassign_model: %s\n", why); free(a); return NULL; }
	return a;
}

void cellassign_model_annot_free(void *h)
{
	svg_cell_annot_free(h);
	free(h);
}

/* -> 0, or the builder's refusal */
int cellassign_model_barcodes(const char *whitelist, uint64_t nwl, int L, const char *reads, uint64_t n, int32_t *out)
{
	svg_cell_bcodes b;
	char why[256];
	const char **ptr = malloc(sizeof(char *) * (nwl ? nwl : 1));
	for (uint64_t i = 0; i < nwl; i++) ptr[i] = whitelist + i * (size_t)(L + 1);
	const int rc = svg_cell_bcodes_build(ptr, nwl, L, &b, why, sizeof why);
	free(ptr);
	if (rc) { fprintf(stderr, "cellassign_model: %s\n", why); return rc; }
	for (uint64_t i = 0; i < n; i++) out[i] = cellassign_model_barcode(&b, whitelist, reads + i * (size_t)(L + 1));
	svg_cell_bcodes_free(&b);
	return 0;
}
