/* TEST INFRASTRUCTURE ONLY: the voting step of the reference's cellCounts for a list of reads,
 * run with the reference's own prefill_votes (cell-counts.c:432-489) and
 * cellCounts_process_copy_ptrs_to_votes (cell-counts.c:2786-2881), compiled from the reference
 * source where it lies (this file #includes it; nothing is copied), over a subread-buildindex
 * index block.  Built and run by make_cellvote_golden.py only; the binary is never kept.
 *
 *   ref-cellvote <index prefix> <total subreads> <reads.txt> <heads.bin> <slots.bin> <keys.bin>
 *
 * reads.txt holds one read per line (an empty line is a read of no bases).  Per read, in
 * svg_cell_vote_batch's record format (include/subread_vote.h): one 32-byte head to heads.bin and
 * its used slots, rows 0..16 and slots 0..items-1, 56 bytes each, to slots.bin.  keys.bin lists
 * every looked-up key as five u32 (read, strand, offset, key, run length) for the generator's
 * cross-check and its edge counts. */
#define main cellcounts_unused_main
#include REF_CELL_COUNTS
#undef main

typedef struct {
	uint64_t first_slot;
	uint16_t n_slots;
	int16_t max_vote;
	int16_t applied_subreads;
	uint8_t items[GENE_SCRNA_VOTE_TABLE_SIZE];
	uint8_t pad;
} cv_head;

typedef struct {
	uint32_t pos;
	int16_t mask;
	int16_t votes;
	int16_t coverage_start, coverage_end;
	uint8_t toli;
	uint8_t pad;
	int16_t indel_recorder[MAX_INDEL_TOLERANCE * 3];
} cv_slot;

int main(int argc, char **argv)
{
	if (argc != 7) { fprintf(stderr, "usage: %s prefix total_subreads reads.txt heads.bin slots.bin keys.bin\n", argv[0]); return 2; }
	if (sizeof(cv_head) != 32 || sizeof(cv_slot) != 56) { fprintf(stderr, "record layout\n"); return 1; }
	char tab[1030];
	snprintf(tab, sizeof tab, "%s.00.b.tab", argv[1]);
	gehash_t table;
	if (gehash_load(&table, tab)) { fprintf(stderr, "cannot load %s\n", tab); return 1; }
	cellcounts_global_t *ctx = calloc(1, sizeof *ctx);
	/* what the two functions and the plan read: the defaults of cellCounts_args_context
	 * (cell-counts.c:521,526) and --subreadsPerRead with its clamp (:547) */
	ctx->current_index = &table;
	ctx->max_indel_length = 5;
	ctx->total_subreads_per_read = min(SCRNA_SUBREADS_HARD_LIMIT, max(7, atoi(argv[2])));
	FILE *fr = fopen(argv[3], "r"), *fh = fopen(argv[4], "wb"), *fs = fopen(argv[5], "wb"), *fk = fopen(argv[6], "wb");
	if (!fr || !fh || !fs || !fk) { fprintf(stderr, "cannot open a file\n"); return 1; }
	temp_votes_per_read_t *ptrs = calloc(1, sizeof *ptrs);
	gene_sc_vote_t *vote = calloc(1, sizeof *vote);
	char line[1024], text[2 * MAX_SCRNA_READ_LENGTH + 2];
	const int gap = table.index_gap;
	uint64_t nslots = 0;
	unsigned int rno = 0;
	for (; fgets(line, sizeof line, fr); rno++) {
		int len = (int)strcspn(line, "\r\n");
		if (len > MAX_SCRNA_READ_LENGTH) { fprintf(stderr, "read %u: %d bases\n", rno, len); return 1; }
		cv_head h;
		memset(&h, 0, sizeof h);
		if (len >= 16) {   /* a shorter read is skipped (cell-counts.c:3077): a zero head */
			h.first_slot = nslots;
			/* the subread plan of cellCounts_do_voting (cell-counts.c:3079-3082) */
			int span = (len - 15 - gap) << 16;
			int step = span / (ctx->total_subreads_per_read - 1);
			if (step < (gap << 16)) step = gap << 16;
			int applied = 1 + span / step;
			memcpy(text, line, len);
			text[len] = 0;
			/* the second strand's text, as :3117-3120 make it */
			char *rev = text + MAX_SCRNA_READ_LENGTH + 1;
			strcpy(rev, text);
			reverse_read(rev, len, GENE_SPACE_BASE);
			for (int strand = 0; strand < 2; strand++) {
				const char *t = strand ? rev : text;
				gehash_key_t key = 0;
				int next = 0;   /* bases shifted into the key so far */
				for (int k = 0; k < applied; k++) {
					int off = (step * k) >> 16;
					for (; next < off + 16; next++) key = (key << 2) | base2int(t[next]);
					prefill_votes(&table, ptrs, applied, key, off, k, strand);
					unsigned int rec[5] = {rno, (unsigned)strand, (unsigned)off, key,
					                       (unsigned)ptrs->votes[k + applied * strand]};
					fwrite(rec, 4, 5, fk);
				}
			}
			cellCounts_process_copy_ptrs_to_votes(ctx, 0, ptrs, vote, applied, "r");
			h.max_vote = vote->max_vote;
			h.applied_subreads = (int16_t)applied;
			for (int i = 0; i < GENE_SCRNA_VOTE_TABLE_SIZE; i++) {
				h.items[i] = (uint8_t)vote->items[i];
				for (int j = 0; j < vote->items[i]; j++) {
					cv_slot s;
					memset(&s, 0, sizeof s);
					s.pos = vote->pos[i][j];
					s.mask = (int16_t)vote->masks[i][j];
					s.votes = vote->votes[i][j];
					s.coverage_start = vote->coverage_start[i][j];
					s.coverage_end = vote->coverage_end[i][j];
					s.toli = (uint8_t)vote->toli[i][j];
					for (int t = 0; t < vote->toli[i][j]; t++) s.indel_recorder[t] = vote->indel_recorder[i][j][t];
					fwrite(&s, sizeof s, 1, fs);
					h.n_slots++;
				}
			}
			nslots += h.n_slots;
		}
		fwrite(&h, sizeof h, 1, fh);
	}
	fclose(fr); fclose(fh); fclose(fs); fclose(fk);
	return 0;
}
