/* TEST INFRASTRUCTURE ONLY: the reference's cellCounts_select_and_write_alignments
 * (cell-counts.c:2648-2719) for a list of reads, compiled from the reference source where it lies
 * (this file #includes it; nothing is copied).  The vote table and read_bin are made as
 * ref_cellvote.c makes them (the reference's prefill_votes and
 * cellCounts_process_copy_ptrs_to_votes), the .array image is loaded with gvindex_load.
 * cellCounts_write_read_in_batch_bin is replaced by a recorder: make_cellalign_golden.py compiles
 * this file twice, once as the harness (-fPIC, the reference's writer weakened with objcopy) and
 * once with -DCELLALIGN_RECORDER as the strong definition.  The binary is never kept.
 *
 *   ref-cellalign <index prefix> <reads.txt> <exons.bin> <heads.bin> <alns.bin> total_subreads
 *                 min_votes max_diff max_mismatch min_mapped_length max_reported
 *
 * exons.bin: pairs of u32 (inclusive linear start, stop), as linear_gene_position gives them.
 *
 * One thing here is restated, not the reference's own code: the fill of the two exon planes in
 * main().  The reference's fill (cell-counts.c:941-959) sits inside its annotation loader, which
 * reads a feature table, so it cannot be called on a list of intervals; main() repeats its two
 * loops and its > 0xffffff00 refusal.  The weights in the fixtures are the reference's only as
 * far as that restatement is right.  Everything downstream of the planes, the weight lookup
 * (cellCounts_calculate_pos_weight) included, is the reference's code.
 *
 * Output in svg_cell_align_batch's record format (include/subread_vote.h). */
#ifdef CELLALIGN_RECORDER
void cellalign_record(int reporting_index);
void cellCounts_write_read_in_batch_bin(void *cct_context, int thread_no, int reporting_index, char *read_name, char *read_text,
                                        char *qual_text, char *raw_text, char *raw_qual, int rlen)
{
	cellalign_record(reporting_index);
}
#else
#define main cellcounts_unused_main
#include REF_CELL_COUNTS
#undef main

#define CIGAR_FIELD 108
typedef struct {
	uint64_t first_record;
	uint16_t n_records, multi_alignment_no;
	uint32_t pad;
} ca_head;
typedef struct {
	int64_t score;
	uint32_t position;
	int16_t flags, mapq;
	int32_t editing_distance;
	char cigar[CIGAR_FIELD];
} ca_aln;

static cellcounts_global_t *ctx;
static FILE *fa;
static ca_head head;
static uint64_t nrec;

void cellalign_record(int reporting_index)
{
	cellcounts_align_thread_t *t = ctx->all_thread_contexts;
	head.multi_alignment_no = (uint16_t)t->reporting_multi_alignment_no;
	if (reporting_index < 0) return;   /* written as unmapped: no record */
	ca_aln a;
	memset(&a, 0, sizeof a);
	a.score = t->reporting_scores[reporting_index];
	a.position = t->reporting_positions[reporting_index];
	a.flags = (int16_t)t->reporting_flags[reporting_index];
	a.mapq = (int16_t)t->reporting_mapq[reporting_index];
	a.editing_distance = t->reporting_editing_distance[reporting_index];
	if (strlen(t->reporting_cigars[reporting_index]) >= CIGAR_FIELD) { fprintf(stderr, "a CIGAR longer than its field\n"); exit(1); }
	strcpy(a.cigar, t->reporting_cigars[reporting_index]);
	fwrite(&a, sizeof a, 1, fa);
	if (!head.n_records) head.first_record = nrec;
	head.n_records++;
	nrec++;
}

int main(int argc, char **argv)
{
	if (argc != 12) { fprintf(stderr, "usage: %s prefix reads.txt exons.bin heads.bin alns.bin total min_votes max_diff max_mm min_len max_rep\n", argv[0]); return 2; }
	if (sizeof(ca_head) != 16 || sizeof(ca_aln) != 128) { fprintf(stderr, "record layout\n"); return 1; }
	char name[1030];
	snprintf(name, sizeof name, "%s.00.b.tab", argv[1]);
	gehash_t table;
	if (gehash_load(&table, name)) { fprintf(stderr, "cannot load %s\n", name); return 1; }
	snprintf(name, sizeof name, "%s.00.b.array", argv[1]);
	gene_value_index_t value_index;
	if (gvindex_load(&value_index, name)) { fprintf(stderr, "cannot load %s\n", name); return 1; }
	ctx = calloc(1, sizeof *ctx);
	ctx->all_thread_contexts = calloc(1, sizeof(cellcounts_align_thread_t));
	ctx->current_index = &table;
	ctx->value_index = &value_index;
	/* the defaults of cellCounts_args_context (:517-529), the options' clamps (:538-569) and the fix-up (:604) */
	ctx->max_indel_length = 5;
	ctx->max_distinct_top_vote_numbers = 3;
	ctx->max_voting_simples = 3;
	ctx->total_subreads_per_read = min(SCRNA_SUBREADS_HARD_LIMIT, max(7, atoi(argv[6])));
	ctx->min_votes_per_mapped_read = min(64, max(1, atoi(argv[7])));
	ctx->max_differential_from_top_vote_number = min(30, max(1, atoi(argv[8])));
	ctx->max_mismatching_bases_in_reads = min(100, max(0, atoi(argv[9])));
	ctx->min_mapped_length_for_mapped_read = min(MAX_SCRNA_READ_LENGTH, max(-1, atoi(argv[10])));
	ctx->max_reported_alignments_per_read = min(SCRNA_HIGHEST_REPORTED_ALIGNMENTS, max(1, atoi(argv[11])));
	ctx->max_voting_simples = max(ctx->max_voting_simples, ctx->max_reported_alignments_per_read);
	/* the two planes, sized and filled as :1381 and :938-959 do */
	const size_t plane = (size_t)(4096 / 8) * 1024 * 1024;
	ctx->exonic_region_bitmap = calloc(plane * 2, 1);
	FILE *fr = fopen(argv[2], "r"), *fe = fopen(argv[3], "rb"), *fh = fopen(argv[4], "wb");
	fa = fopen(argv[5], "wb");
	if (!ctx->exonic_region_bitmap || !fr || !fe || !fh || !fa) { fprintf(stderr, "cannot open a file\n"); return 1; }
	unsigned int ex[2];
	while (fread(ex, 4, 2, fe) == 2) {
		unsigned int i;
		if (ex[0] > 0xffffff00 || ex[1] > 0xffffff00) continue;
		for (i = ex[0]; i <= ex[1]; i++) ctx->exonic_region_bitmap[i / 8] |= (1 << (i % 8));
		for (i = ex[0] - 100; i <= ex[1] + 100; i++) ctx->exonic_region_bitmap[i / 8 + plane] |= (1 << (i % 8));
	}
	temp_votes_per_read_t *ptrs = calloc(1, sizeof *ptrs);
	gene_sc_vote_t *vote = calloc(1, sizeof *vote);
	char line[1024], text[2 * MAX_SCRNA_READ_LENGTH + 2], qual[2 * MAX_SCRNA_READ_LENGTH + 2], read_bin[REVERSED_READ_BIN_OFFSET * 2];
	const int gap = table.index_gap;
	while (fgets(line, sizeof line, fr)) {
		int len = (int)strcspn(line, "\r\n");
		if (len > MAX_SCRNA_READ_LENGTH) { fprintf(stderr, "a read of %d bases\n", len); return 1; }
		memset(&head, 0, sizeof head);
		int applied = 0, step = 0;
		if (len >= 16) {
			int span = (len - 15 - gap) << 16;
			step = span / (ctx->total_subreads_per_read - 1);
			if (step < (gap << 16)) step = gap << 16;
			applied = 1 + span / step;
		}
		/* one subread per strand: find_subread_end would divide by zero; the library reports nothing */
		if (applied >= 2) {
			memcpy(text, line, len);
			text[len] = 0;
			char *rev = text + MAX_SCRNA_READ_LENGTH + 1;
			strcpy(rev, text);
			reverse_read(rev, len, GENE_SPACE_BASE);
			memset(qual, 'I', sizeof qual);
			qual[len] = 0;
			qual[MAX_SCRNA_READ_LENGTH + 1] = 0;
			memset(read_bin, 0, sizeof read_bin);
			for (int strand = 0; strand < 2; strand++) {
				const char *t = strand ? rev : text;
				/* read_bin of :3091-3105: base2int codes, LSB first */
				for (int i = 0; i < len; i++) read_bin[strand * REVERSED_READ_BIN_OFFSET + i / 4] |= base2int(t[i]) << (i % 4 * 2);
				gehash_key_t key = 0;
				int next = 0;
				for (int k = 0; k < applied; k++) {
					int off = (step * k) >> 16;
					for (; next < off + 16; next++) key = (key << 2) | base2int(t[next]);
					prefill_votes(&table, ptrs, applied, key, off, k, strand);
				}
			}
			cellCounts_process_copy_ptrs_to_votes(ctx, 0, ptrs, vote, applied, "r");
			cellCounts_select_and_write_alignments(ctx, 0, vote, "r", text, read_bin, qual, len, applied);
		}
		fwrite(&head, sizeof head, 1, fh);
	}
	fclose(fr); fclose(fe); fclose(fh); fclose(fa);
	return 0;
}
#endif
