/* svg_cell_annot.h -- the host tables behind svg_cell_set_annotation and svg_cell_set_barcodes
 * (svg_cell_annot.c: plain C, no HIP, so that a program of its own can link it). */
#ifndef SVG_CELL_ANNOT_H
#define SVG_CELL_ANNOT_H
#include <stdint.h>
#include "subread_vote.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVG_CELL_REV_BUCKET 131072u   /* REVERSE_TABLE_BUCKET_LENGTH */

/* what cellCounts_sort_feature_info (cell-counts.c:1099-1251) leaves, contig by contig in the order
 * of the index's .reads table */
typedef struct svg_cell_annot {
	uint32_t n_features, n_blocks, n_contigs, rev_words;
	uint32_t *start, *end;          /* features_sorted_start / _stop */
	int32_t  *gene;                 /* features_sorted_geneid */
	uint8_t  *strand;               /* features_sorted_strand */
	uint32_t *block_end, *block_min, *block_max;   /* block_end_index, block_min_start, block_max_end */
	uint32_t *chro_len;             /* chro_possible_length */
	uint32_t *chro_block_end;       /* chro_block_table_end */
	uint32_t *rev_first;            /* the contig's reverse table: rev[rev_first[c] .. + chro_len[c] / 131072 + 2) */
	uint32_t *rev;
	uint32_t *exon_start, *exon_stop;   /* linear_gene_position of start and end, annotation order (:939-940) */
} svg_cell_annot;

/* chr_end: the .reads offsets.  0, or SVG_E_ARG / SVG_E_NOMEM with the reason written into whybuf */
int  svg_cell_annot_build(const svg_cell_feature *f, uint64_t n, const uint32_t *chr_end, uint32_t n_chr, int padding,
                          svg_cell_annot *out, char *whybuf, size_t whylen);
void svg_cell_annot_free(svg_cell_annot *a);

/* the whitelist image: codes in whitelist order (position i in bits 2i .. 2i + 1, base2int codes)
 * and the two half-key lists as CSR rows of whitelist numbers, ascending in each row */
typedef struct svg_cell_bcodes {
	uint32_t n, length, rows;       /* rows = 4 ^ (length / 2) */
	uint32_t *code;
	uint32_t *frow, *srow;          /* rows + 1 */
	uint32_t *fent, *sent;          /* n */
} svg_cell_bcodes;

int  svg_cell_bcodes_build(const char *const *barcodes, uint64_t n, int length, svg_cell_bcodes *out, char *whybuf, size_t whylen);
void svg_cell_bcodes_free(svg_cell_bcodes *b);

#ifdef __cplusplus
}
#endif
#endif
