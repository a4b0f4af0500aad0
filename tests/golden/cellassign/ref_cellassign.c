/* TEST INFRASTRUCTURE ONLY: the reference's cellCounts_write_read_in_batch_bin (cell-counts.c:
 * 2061-2088) behind its cellCounts_select_and_write_alignments, for a list of reads, compiled from
 * the reference source where it lies (this file #includes it; nothing is copied).  The annotation
 * goes through the reference's own cellCounts_load_annotations (load_features_annotation with
 * features_load_one_line, which also fills the two exon planes, and cellCounts_sort_feature_info),
 * the whitelist through cellCounts_make_barcode_HT_table; each read is voted and aligned as
 * ref_cellalign.c does.  cellCounts_vote_and_add_count is replaced by a recorder:
 * make_cellassign_golden.py compiles this file twice, once as the harness (-fPIC, the reference's
 * function weakened with objcopy) and once with -DCELLASSIGN_RECORDER as the strong definition.
 * The binary is never kept.
 *
 *   ref-cellassign <index prefix> <reads.txt> <features.bin> <whitelist.txt> <out dir> allow_multi
 *                  total_subreads min_votes max_diff max_mismatch min_mapped_length max_reported
 *
 * reads.txt: "<read> <cell barcode>" per line.  features.bin: svg_cell_feature records (20 bytes);
 * the harness writes them as a SAF file with the contig names of the index and genes "g<number>".
 * Output: heads.bin, alns.bin, hits.bin, genes.bin, bc.bin in the library's record formats, flags.bin
 * (one byte per read: 1 = a call inside the loop of :2700-2715 was turned into an unmapped one, so
 * the alignment record behind it is not known here; the maker drops such reads) and tables.bin, the
 * reference's tables: 4 u64 (features, blocks, contigs, reverse-table words), then as i64
 * features_sorted_start, _stop, then u8 strand, i32 geneid, i64 block_end_index, block_min_start,
 * block_max_end, then per contig u32 chro_possible_length, chro_block_table_end, bins, and the
 * reverse tables back to back. */
#ifdef CELLASSIGN_RECORDER
void cellassign_record(char *chro_name, int chro_pos, int reporting_index, int nhits);
void cellCounts_vote_and_add_count(void *cct_context, int thread_no, char *read_name, int rlen, char *read_text, char *qual_text,
                                   char *raw_text, char *raw_qual, char *chro_name, int chro_pos, int reporting_index, int nhits,
                                   int multi_mapping_number, int this_multi_mapping_i, int editing_dist)
{
	cellassign_record(chro_name, chro_pos, reporting_index, nhits);
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
typedef struct {
	int32_t contig, chro_pos;
	uint32_t nhits, pad;
	uint64_t first_gene;
} ca_hit;
typedef struct {
	uint32_t contig, start, end;
	int32_t gene;
	uint8_t neg, pad[3];
} ca_feature;

static cellcounts_global_t *ctx;
static FILE *fa, *fhit, *fgene;
static ca_head head;
static uint64_t nrec, ngene;
static int lost;

void cellassign_record(char *chro_name, int chro_pos, int reporting_index, int nhits)
{
	cellcounts_align_thread_t *t = ctx->all_thread_contexts;
	head.multi_alignment_no = (uint16_t)t->reporting_multi_alignment_no;
	if (reporting_index < 0) {
		if (t->reporting_this_alignment_no != -7) lost = 1;   /* inside the loop: locate_gene_position refused it */
		return;
	}
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
	ca_hit h;
	memset(&h, 0, sizeof h);
	h.contig = (int32_t)((chro_name - ctx->chromosome_table.read_names) / MAX_CHROMOSOME_NAME_LEN);
	h.chro_pos = chro_pos;
	/* the rule of :1982, which the replaced function applies */
	if (nhits > 1 && !ctx->allow_multi_overlapping_reads) nhits = 0;
	h.nhits = (uint32_t)nhits;
	if (nhits) h.first_gene = ngene;
	for (int i = 0; i < nhits; i++) {
		int32_t g = (int32_t)t->hits_indices[i];
		fwrite(&g, 4, 1, fgene);
		ngene++;
	}
	fwrite(&h, sizeof h, 1, fhit);
	if (!head.n_records) head.first_record = nrec;
	head.n_records++;
	nrec++;
}

static FILE *out_file(const char *dir, const char *name)
{
	char fn[1200];
	snprintf(fn, sizeof fn, "%s/%s", dir, name);
	FILE *f = fopen(fn, "wb");
	if (!f) { fprintf(stderr, "cannot write %s\n", fn); exit(1); }
	return f;
}

int main(int argc, char **argv)
{
	if (argc != 13) { fprintf(stderr, "usage: %s prefix reads.txt features.bin whitelist.txt outdir allow total min_votes max_diff max_mm min_len max_rep\n", argv[0]); return 2; }
	if (sizeof(ca_head) != 16 || sizeof(ca_aln) != 128 || sizeof(ca_hit) != 24 || sizeof(ca_feature) != 20) { fprintf(stderr, "record layout\n"); return 1; }
	char name[1200];
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
	strcpy(ctx->index_prefix, argv[1]);
	if (load_offsets(&ctx->chromosome_table, argv[1])) { fprintf(stderr, "cannot load the offsets\n"); return 1; }
	const char *dir = argv[5];
	ctx->allow_multi_overlapping_reads = atoi(argv[6]);
	ctx->max_indel_length = 5;
	ctx->max_distinct_top_vote_numbers = 3;
	ctx->max_voting_simples = 3;
	ctx->total_subreads_per_read = min(SCRNA_SUBREADS_HARD_LIMIT, max(7, atoi(argv[7])));
	ctx->min_votes_per_mapped_read = min(64, max(1, atoi(argv[8])));
	ctx->max_differential_from_top_vote_number = min(30, max(1, atoi(argv[9])));
	ctx->max_mismatching_bases_in_reads = min(100, max(0, atoi(argv[10])));
	ctx->min_mapped_length_for_mapped_read = min(MAX_SCRNA_READ_LENGTH, max(-1, atoi(argv[11])));
	ctx->max_reported_alignments_per_read = min(SCRNA_HIGHEST_REPORTED_ALIGNMENTS, max(1, atoi(argv[12])));
	ctx->max_voting_simples = max(ctx->max_voting_simples, ctx->max_reported_alignments_per_read);
	ctx->exonic_region_bitmap = calloc((size_t)(4096 / 8) * 1024 * 1024 * 2, 1);   /* :1381 */
	if (!ctx->exonic_region_bitmap) { fprintf(stderr, "out of memory\n"); return 1; }

	/* the SAF file, then the reference's own loader and sort */
	snprintf(ctx->features_annotation_file, sizeof ctx->features_annotation_file, "%s/annot.saf", dir);
	ctx->features_annotation_file_type = FILE_TYPE_RSUBREAD;
	FILE *ff = fopen(argv[3], "rb"), *fs = fopen(ctx->features_annotation_file, "w");
	if (!ff || !fs) { fprintf(stderr, "cannot open the features\n"); return 1; }
	fprintf(fs, "GeneID\tChr\tStart\tEnd\tStrand\n");
	ca_feature ft;
	while (fread(&ft, sizeof ft, 1, ff) == 1)
		fprintf(fs, "g%d\t%s\t%u\t%u\t%c\n", ft.gene, ctx->chromosome_table.read_names + (size_t)ft.contig * MAX_CHROMOSOME_NAME_LEN, ft.start, ft.end,
		        ft.neg ? '-' : '+');
	fclose(ff); fclose(fs);
	if (cellCounts_load_annotations(ctx)) { fprintf(stderr, "cellCounts_load_annotations failed\n"); return 1; }

	/* the tables */
	{
		FILE *f = out_file(dir, "tables.bin");
		const gene_offset_t *ot = &ctx->chromosome_table;
		uint64_t hdr[4] = {(uint64_t)ctx->all_features_array->numOfElements, 0, (uint64_t)ot->total_offsets, 0};
		for (int c = 0; c < ot->total_offsets; c++) {
			fc_chromosome_index_info *ci = HashTableGet(ctx->chromosome_exons_table, ot->read_names + (size_t)c * MAX_CHROMOSOME_NAME_LEN);
			if (ci->chro_block_table_end > hdr[1]) hdr[1] = ci->chro_block_table_end;
			hdr[3] += ci->chro_possible_length / REVERSE_TABLE_BUCKET_LENGTH + 2;
		}
		fwrite(hdr, 8, 4, f);
		fwrite(ctx->features_sorted_start, 8, hdr[0], f);
		fwrite(ctx->features_sorted_stop, 8, hdr[0], f);
		fwrite(ctx->features_sorted_strand, 1, hdr[0], f);
		fwrite(ctx->features_sorted_geneid, 4, hdr[0], f);
		fwrite(ctx->block_end_index, 8, hdr[1], f);
		fwrite(ctx->block_min_start, 8, hdr[1], f);
		fwrite(ctx->block_max_end, 8, hdr[1], f);
		for (int c = 0; c < ot->total_offsets; c++) {
			fc_chromosome_index_info *ci = HashTableGet(ctx->chromosome_exons_table, ot->read_names + (size_t)c * MAX_CHROMOSOME_NAME_LEN);
			uint32_t v[3] = {ci->chro_possible_length, ci->chro_block_table_end, ci->chro_possible_length / REVERSE_TABLE_BUCKET_LENGTH + 2};
			fwrite(v, 4, 3, f);
		}
		for (int c = 0; c < ot->total_offsets; c++) {
			fc_chromosome_index_info *ci = HashTableGet(ctx->chromosome_exons_table, ot->read_names + (size_t)c * MAX_CHROMOSOME_NAME_LEN);
			fwrite(ci->reverse_table_start_index, 4, ci->chro_possible_length / REVERSE_TABLE_BUCKET_LENGTH + 2, f);
		}
		fclose(f);
	}

	/* the whitelist */
	ctx->cell_barcodes_array = ArrayListCreate(1000);
	char line[1024];
	FILE *fw = fopen(argv[4], "r");
	if (!fw) { fprintf(stderr, "cannot open the whitelist\n"); return 1; }
	while (fgets(line, sizeof line, fw)) {
		line[strcspn(line, "\r\n")] = 0;
		if (line[0]) ArrayListPush(ctx->cell_barcodes_array, strdup(line));
	}
	fclose(fw);
	if (cellCounts_make_barcode_HT_table(ctx)) return 1;

	FILE *fr = fopen(argv[2], "r"), *fh = out_file(dir, "heads.bin"), *fb = out_file(dir, "bc.bin"), *fl = out_file(dir, "flags.bin");
	fa = out_file(dir, "alns.bin"); fhit = out_file(dir, "hits.bin"); fgene = out_file(dir, "genes.bin");
	if (!fr) { fprintf(stderr, "cannot open the reads\n"); return 1; }
	temp_votes_per_read_t *ptrs = calloc(1, sizeof *ptrs);
	gene_sc_vote_t *vote = calloc(1, sizeof *vote);
	char text[2 * MAX_SCRNA_READ_LENGTH + 2], qual[2 * MAX_SCRNA_READ_LENGTH + 2], read_bin[REVERSED_READ_BIN_OFFSET * 2], cbc[64];
	const int gap = table.index_gap;
	while (fgets(line, sizeof line, fr)) {
		int len = (int)strcspn(line, " \r\n");
		if (len > MAX_SCRNA_READ_LENGTH || line[len] != ' ') { fprintf(stderr, "a bad read line\n"); return 1; }
		/* the barcode as the read name holds it: the UMI follows it */
		char *b = line + len + 1;
		int bl = (int)strcspn(b, "\r\n");
		if (bl > 32) { fprintf(stderr, "a long barcode\n"); return 1; }
		memcpy(cbc, b, bl);
		strcpy(cbc + bl, "ACGTACGTACGT");
		int32_t bcno = cellCounts_get_cellbarcode_no(ctx, 0, cbc);
		fwrite(&bcno, 4, 1, fb);
		memset(&head, 0, sizeof head);
		lost = 0;
		int applied = 0, step = 0;
		if (len >= 16) {
			int span = (len - 15 - gap) << 16;
			step = span / (ctx->total_subreads_per_read - 1);
			if (step < (gap << 16)) step = gap << 16;
			applied = 1 + span / step;
		}
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
			ctx->all_thread_contexts->reporting_this_alignment_no = -7;   /* stays so on the unmapped branch of :2716 */
			cellCounts_select_and_write_alignments(ctx, 0, vote, "r", text, read_bin, qual, len, applied);
		}
		fwrite(&head, sizeof head, 1, fh);
		fputc(lost, fl);
	}
	fclose(fr); fclose(fh); fclose(fa); fclose(fhit); fclose(fgene); fclose(fb); fclose(fl);
	return 0;
}
#endif
