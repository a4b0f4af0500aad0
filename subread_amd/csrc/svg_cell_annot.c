/* svg_cell_annot.c -- the host side of svg_cell_set_annotation and svg_cell_set_barcodes: the tables
 * of cellCounts_sort_feature_info (cell-counts.c:1099-1251) and of cellCounts_make_barcode_HT_table
 * (:272-304), in plain C without HIP so that a program of its own can link this file. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "svg_cell_annot.h"

typedef struct { uint32_t start, end; int32_t gene; uint8_t strand; } feat_t;

/* basic_sort_run, core.c:4716-4729: a selection sort that exchanges, so not stable */
static void basic_sort_run(feat_t *a, int start, int items)
{
	for (int i = start; i < start + items - 1; i++) {
		int min_j = i;
		for (int j = i + 1; j < start + items; j++)
			if (a[min_j].start > a[j].start) min_j = j;
		if (i != min_j) { feat_t t = a[i]; a[i] = a[min_j]; a[min_j] = t; }
	}
}

/* cellCounts_feature_merge, :992-1047: on equal starts the second run's item goes first */
static void feature_merge(feat_t *a, feat_t *tmp, int start, int items, int items2)
{
	const int total = items + items2;
	int r1 = start, r2 = start + items;
	for (int w = 0; w < total; w++) {
		if (r1 >= start + items || (r2 < start + total && a[r1].start >= a[r2].start)) tmp[w] = a[r2++];
		else tmp[w] = a[r1++];
	}
	memcpy(a + start, tmp, sizeof(feat_t) * (size_t)total);
}

/* merge_sort_run, core.c:4736-4749 */
static void merge_sort_run(feat_t *a, feat_t *tmp, int start, int items)
{
	if (items > 11) {
		const int half = items / 2;
		merge_sort_run(a, tmp, start, half);
		merge_sort_run(a, tmp, start + half, items - half);
		feature_merge(a, tmp, start, half, items - half);
	} else basic_sort_run(a, start, items);
}

void svg_cell_annot_free(svg_cell_annot *a)
{
	if (!a) return;
	free(a->start); free(a->end); free(a->gene); free(a->strand);
	free(a->block_end); free(a->block_min); free(a->block_max);
	free(a->chro_len); free(a->chro_block_end); free(a->rev_first); free(a->rev);
	free(a->exon_start); free(a->exon_stop);
	memset(a, 0, sizeof *a);
}

#define WHY(...) do { snprintf(whybuf, whylen, __VA_ARGS__); } while (0)

int svg_cell_annot_build(const svg_cell_feature *f, uint64_t n, const uint32_t *chr_end, uint32_t n_chr, int padding,
                         svg_cell_annot *out, char *whybuf, size_t whylen)
{
	memset(out, 0, sizeof *out);
	if (n > 0x7fffffffu) { WHY("%llu features (at most 2^31 - 1)", (unsigned long long)n); return SVG_E_ARG; }
	/* cellCounts_load_annotations :1269-1280 and features_load_one_line :918-936: a stub per contig
	 * of the index, its length the difference of the .reads offsets (the padding counts), raised to
	 * end + 1 of any feature; the reverse table first counts the features by the bucket of their start */
	uint32_t *chro_len = calloc(n_chr ? n_chr : 1, 4), *count = calloc((size_t)n_chr + 1, 4), *alloc = calloc(n_chr ? n_chr : 1, 4);
	uint32_t *rev_first = calloc((size_t)n_chr + 1, 4);
	feat_t *a = malloc(sizeof(feat_t) * (n ? n : 1)), *tmp = malloc(sizeof(feat_t) * (n ? n : 1));
	out->exon_start = malloc(4 * (n ? n : 1));
	out->exon_stop = malloc(4 * (n ? n : 1));
	uint32_t *rev = NULL, *fill = NULL, *bend = NULL, *bmin = NULL, *bmax = NULL;
	int rc = SVG_E_NOMEM;
	if (!chro_len || !count || !alloc || !rev_first || !a || !tmp || !out->exon_start || !out->exon_stop) { WHY("out of host memory"); goto done; }
	rc = SVG_E_ARG;
	for (uint32_t c = 0; c < n_chr; c++) {
		chro_len[c] = chr_end[c] - (c ? chr_end[c - 1] : 0);
		alloc[c] = (uint32_t)(((uint64_t)chro_len[c] + 1024 * 1024) / SVG_CELL_REV_BUCKET + 2);   /* :1277-1278 */
	}
	for (uint64_t i = 0; i < n; i++) {
		const uint32_t c = f[i].contig;
		if (c >= n_chr) { WHY("feature %llu: contig %u of %u", (unsigned long long)i, c, n_chr); goto done; }
		if (f[i].start > f[i].end) { WHY("feature %llu ends before it starts", (unsigned long long)i); goto done; }
		if (f[i].is_negative_strand > 1) { WHY("feature %llu: strand %d (0 or 1)", (unsigned long long)i, f[i].is_negative_strand); goto done; }
		/* the reference's table has alloc[c] buckets and is written at start / 131072 (:935) and read
		 * up to chro_possible_length / 131072 + 1 (:1175-1181): a feature beyond it is outside its contract */
		if (f[i].end == 0xffffffffu || (uint64_t)(f[i].end + 1u) / SVG_CELL_REV_BUCKET + 2 > alloc[c]) {
			WHY("feature %llu ends at %u, more than 1 Mbase beyond its contig of %u bases (the reference writes past its reverse table)",
			    (unsigned long long)i, f[i].end, chro_len[c]);
			goto done;
		}
		if (chro_len[c] < f[i].end + 1u) chro_len[c] = f[i].end + 1u;   /* :920 */
		count[c + 1]++;
		const uint32_t lin = (c ? chr_end[c - 1] : 0) + (uint32_t)padding;   /* linear_gene_position, gene-algorithms.c:419-433 */
		out->exon_start[i] = lin + f[i].start;
		out->exon_stop[i] = lin + f[i].end;
	}
	uint64_t words = 0;
	for (uint32_t c = 0; c < n_chr; c++) {
		count[c + 1] += count[c];
		rev_first[c] = (uint32_t)words;
		words += chro_len[c] / SVG_CELL_REV_BUCKET + 2;
		if (words > 0xffffffffu) { WHY("reverse tables of more than 2^32 words"); goto done; }
	}
	rc = SVG_E_NOMEM;
	rev = calloc(words ? words : 1, 4);
	fill = malloc(4 * ((size_t)n_chr + 1));
	/* (the reference grows the block arrays; a block holds at least one feature) */
	bend = malloc(4 * (n ? n : 1)); bmin = malloc(4 * (n ? n : 1)); bmax = malloc(4 * (n ? n : 1));
	if (!rev || !fill || !bend || !bmin || !bmax) { WHY("out of host memory"); goto done; }
	memcpy(fill, count, 4 * ((size_t)n_chr + 1));
	for (uint64_t i = 0; i < n; i++) {   /* :1153-1170: annotation order within a contig */
		const uint32_t c = f[i].contig;
		feat_t *t = a + fill[c]++;
		t->start = f[i].start; t->end = f[i].end; t->gene = f[i].gene; t->strand = f[i].is_negative_strand;
		rev[rev_first[c] + f[i].start / SVG_CELL_REV_BUCKET]++;   /* :934-935 */
	}
	uint32_t block = 0;
	for (uint32_t c = 0; c < n_chr; c++) {   /* :1173-1242 */
		const uint32_t bins = chro_len[c] / SVG_CELL_REV_BUCKET + 2;
		uint32_t *rt = rev + rev_first[c];
		short *per = malloc(sizeof(short) * bins);
		if (!per) { WHY("out of host memory"); goto done; }
		for (uint32_t b = 0; b < bins; b++) {   /* :1180 */
			int v = (int)(0.9999999 + sqrt(rt[b]));
			per[b] = (short)(v > 1000 ? 1000 : v < 1 ? 1 : v);
		}
		memset(rt, 0xff, 4 * (size_t)bins);
		const uint32_t lo = count[c], hi = count[c + 1];
		merge_sort_run(a, tmp, (int)lo, (int)(hi - lo));
		uint32_t items = 0;
		int64_t mn = 0x7fffffff, mx = 0;
		for (uint32_t s = lo; s <= hi; s++) {
			const int close = s == hi ? items > 0 : items && (items > (uint32_t)per[mn / SVG_CELL_REV_BUCKET] ||
			                  a[s].start / SVG_CELL_REV_BUCKET != (uint32_t)(mn / SVG_CELL_REV_BUCKET));   /* :1202, :1225 */
			if (close) {
				bend[block] = s; bmin[block] = (uint32_t)mn; bmax[block] = (uint32_t)mx;
				/* cellCounts_register_reverse_table :981-990 */
				for (uint32_t x = (uint32_t)(mn / SVG_CELL_REV_BUCKET); x <= (uint32_t)(mx / SVG_CELL_REV_BUCKET); x++)
					if (rt[x] > block) rt[x] = block;
				block++;
				mx = 0; items = 0; mn = 0x7fffffff;
			}
			if (s == hi) break;
			if (a[s].end > mx) mx = a[s].end;
			if (a[s].start < mn) mn = a[s].start;
			items++;
		}
		free(per);
		fill[c] = block;   /* chro_block_table_end :1240 */
	}
	out->start = malloc(4 * (n ? n : 1)); out->end = malloc(4 * (n ? n : 1)); out->gene = malloc(4 * (n ? n : 1));
	out->strand = malloc(n ? n : 1);
	if (!out->start || !out->end || !out->gene || !out->strand) { WHY("out of host memory"); goto done; }
	for (uint64_t i = 0; i < n; i++) { out->start[i] = a[i].start; out->end[i] = a[i].end; out->gene[i] = a[i].gene; out->strand[i] = a[i].strand; }
	out->n_features = (uint32_t)n; out->n_blocks = block; out->n_contigs = n_chr; out->rev_words = (uint32_t)words;
	out->block_end = bend; out->block_min = bmin; out->block_max = bmax;
	out->chro_len = chro_len; out->chro_block_end = fill; out->rev_first = rev_first; out->rev = rev;
	bend = bmin = bmax = chro_len = fill = rev_first = rev = NULL;
	rc = 0;
done:
	free(a); free(tmp); free(count); free(alloc); free(chro_len); free(rev_first); free(rev); free(fill); free(bend); free(bmin); free(bmax);
	if (rc) { free(out->exon_start); free(out->exon_stop); free(out->start); free(out->end); free(out->gene); free(out->strand); memset(out, 0, sizeof *out); }
	return rc;
}

void svg_cell_bcodes_free(svg_cell_bcodes *b)
{
	if (!b) return;
	free(b->code); free(b->frow); free(b->srow); free(b->fent); free(b->sent);
	memset(b, 0, sizeof *b);
}

static int cmp_u32(const void *x, const void *y)
{
	const uint32_t a = *(const uint32_t *)x, b = *(const uint32_t *)y;
	return a < b ? -1 : a > b;
}

int svg_cell_bcodes_build(const char *const *barcodes, uint64_t n, int length, svg_cell_bcodes *out, char *whybuf, size_t whylen)
{
	memset(out, 0, sizeof *out);
	if (length < 2 || length > 16) { WHY("barcodes of %d bases (2..16)", length); return SVG_E_ARG; }
	if (n > 0x0fffffffu) { WHY("%llu barcodes (the reference numbers at most 2^28)", (unsigned long long)n); return SVG_E_ARG; }
	const int half = length / 2;
	const uint32_t rows = 1u << (2 * half);
	uint32_t *sorted = malloc(4 * (n ? n : 1));
	out->code = malloc(4 * (n ? n : 1));
	out->frow = calloc((size_t)rows + 1, 4); out->srow = calloc((size_t)rows + 1, 4);
	out->fent = malloc(4 * (n ? n : 1)); out->sent = malloc(4 * (n ? n : 1));
	uint32_t *fk = malloc(4 * (n ? n : 1)), *sk = malloc(4 * (n ? n : 1));
	int rc = SVG_E_NOMEM;
	if (!sorted || !out->code || !out->frow || !out->srow || !out->fent || !out->sent || !fk || !sk) { WHY("out of host memory"); goto done; }
	rc = SVG_E_ARG;
	for (uint64_t i = 0; i < n; i++) {
		const char *s = barcodes[i];
		if (!s || strlen(s) != (size_t)length) { WHY("barcode %llu has not %d characters", (unsigned long long)i, length); goto done; }
		uint32_t code = 0, f = 0, g = 0;
		for (int k = 0; k < length; k++) {
			/* base2int, subread.h:238 */
			const int b = s[k] == 'A' ? 0 : s[k] == 'G' ? 1 : s[k] == 'C' ? 2 : s[k] == 'T' ? 3 : -1;
			if (b < 0) { WHY("barcode %llu: character '%c' (A, C, G or T)", (unsigned long long)i, s[k]); goto done; }
			code |= (uint32_t)b << (2 * k);
			if (k / 2 < half) { if (k & 1) g |= (uint32_t)b << (k / 2 * 2); else f |= (uint32_t)b << (k / 2 * 2); }
		}
		out->code[i] = sorted[i] = code;
		fk[i] = f; sk[i] = g;
		out->frow[f + 1]++; out->srow[g + 1]++;
	}
	qsort(sorted, n, 4, cmp_u32);
	for (uint64_t i = 1; i < n; i++)
		if (sorted[i] == sorted[i - 1]) { WHY("the whitelist holds a barcode twice"); goto done; }
	for (uint32_t r = 0; r < rows; r++) { out->frow[r + 1] += out->frow[r]; out->srow[r + 1] += out->srow[r]; }
	/* the rows in ascending whitelist order: ArrayListPush in the order of :277 */
	for (uint64_t i = 0; i < n; i++) { out->fent[out->frow[fk[i]]++] = (uint32_t)i; out->sent[out->srow[sk[i]]++] = (uint32_t)i; }
	for (uint32_t r = rows; r > 0; r--) { out->frow[r] = out->frow[r - 1]; out->srow[r] = out->srow[r - 1]; }
	out->frow[0] = out->srow[0] = 0;
	out->n = (uint32_t)n; out->length = (uint32_t)length; out->rows = rows;
	rc = 0;
done:
	free(sorted); free(fk); free(sk);
	if (rc) svg_cell_bcodes_free(out);
	return rc;
}
