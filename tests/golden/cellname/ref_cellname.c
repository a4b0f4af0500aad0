/* Driver over the REFERENCE's read-name functions, used by make_cellname_golden.py only.  It #includes
 * the reference's cell-counts.c where it lies (-DREF_CELL_COUNTS=...; nothing of it is copied here) and
 * calls, per name, the reference's own cellCounts_scan_read_name_str and cellCounts_get_sample_id
 * (which calls its hamming_dist_ATGC_max1 and hamming_dist_ATGC_max1_2p), over a sample_barcode_list
 * built as sheet_convert_ss_to_arr builds it (cell-counts.c:656-666) and a
 * lineno1B_to_sampleno1B_tab; and, per pair of texts, the two Hamming functions directly.
 *
 * The lane number and the choice between the sheet and the "input#" line (:1966-1976) are statements
 * inside cellCounts_vote_and_add_count, which also writes batch files and gzip streams; they are
 * restated below, line for line, around the reference's own calls.  That branch is therefore pinned
 * by this restatement, not by running the function itself.
 *
 *   ref-cellname in.bin out.bin
 * in.bin:  int32 mode (0 BCL, 1 FASTQ), barcode length, UMI length, rows, lines, names, pairs;
 *          rows x { int32 lane, int32 sample, char index[33] }; int32 line_sample[lines] (line i + 1);
 *          names x { int32 length, bytes }; pairs x { char a[33], char b[33] }.
 * out.bin: names x { int32 fields, trimmed length, lane (-1: no lane text), sample, char barcode[16],
 *          char umi[16] }; pairs x { int32 max1, int32 max1_2p }. */
#define main cellcounts_unused_main
#include REF_CELL_COUNTS
#undef main

#pragma pack(push, 1)
typedef struct { int32_t lane, sample; char index[33]; } row_rec;
typedef struct { int32_t fields, trimmed, lane, sample; char bc[16], umi[16]; } out_rec;
#pragma pack(pop)

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	FILE *fp = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	int hdr[7];
	if (!fp || !out || fread(hdr, 4, 7, fp) != 7) return 2;
	const int mode = hdr[0], bl = hdr[1], ul = hdr[2], n_rows = hdr[3], n_lines = hdr[4], n_names = hdr[5], n_pairs = hdr[6];
	cellcounts_global_t *cct_context = calloc(1, sizeof *cct_context);
	cct_context->input_mode = mode ? GENE_INPUT_SCRNA_FASTQ : GENE_INPUT_BCL;
	cct_context->known_cell_barcode_length = bl;
	cct_context->UMI_length = ul;
	cct_context->sample_barcode_list = ArrayListCreate(100);
	cct_context->lineno1B_to_sampleno1B_tab = HashTableCreate(40);
	row_rec *rows = calloc(n_rows + 1, sizeof *rows);
	if (fread(rows, sizeof *rows, n_rows, fp) != (size_t)n_rows) return 2;
	/* one list element per sheet row, in the four-pointer form cellCounts_get_sample_id reads: the lane
	 * and the sample number as pointer values, the index text, and non-NULL for a dual index */
	typedef struct { char *lane_as_ptr, *sample_as_ptr, *text, *is_dual; } sheet_entry;
	sheet_entry *entries = calloc(n_rows + 1, sizeof *entries);
	for (int i = 0; i < n_rows; i++) {
		sheet_entry *e = entries + i;
		e->lane_as_ptr = (char *)(intptr_t)rows[i].lane;
		e->sample_as_ptr = (char *)(intptr_t)rows[i].sample;
		e->text = rows[i].index;
		e->is_dual = strlen(e->text) > 12 ? e->text : NULL;
		ArrayListPush(cct_context->sample_barcode_list, e);
	}
	for (int i = 0; i < n_lines; i++) {
		int32_t s;
		if (fread(&s, 4, 1, fp) != 1) return 2;
		if (s) HashTablePut(cct_context->lineno1B_to_sampleno1B_tab, NULL + (i + 1), NULL + s);
	}
	for (int i = 0; i < n_names; i++) {
		int32_t len;
		if (fread(&len, 4, 1, fp) != 1) return 2;
		char *read_name = calloc(len + 64, 1);
		if (fread(read_name, 1, len, fp) != (size_t)len) return 2;
		char *sample_seq = NULL, *sample_qual = NULL, *BC_qual = NULL, *BC_seq = NULL, *UMI_seq = NULL, *UMI_qual = NULL, *lane_str = NULL, *RG = NULL, *testi;
		int rname_trimmed_len = 0;
		out_rec o;
		memset(&o, 0, sizeof o);
		o.fields = cellCounts_scan_read_name_str(cct_context, NULL, read_name, &sample_seq, &sample_qual, &BC_seq, &BC_qual, &UMI_seq, &UMI_qual,
		                                         &lane_str, &RG, &rname_trimmed_len);
		o.trimmed = rname_trimmed_len;
		o.lane = -1;
		int sample_no = -1;
		if (lane_str) {                                  /* what :1966-1972 do: decimal digits behind the lane text's first character */
			o.lane = 0;
			for (testi = lane_str + 1; *testi >= '0' && *testi <= '9'; testi++) o.lane = o.lane * 10 + (*testi - '0');
			sample_no = cellCounts_get_sample_id(cct_context, sample_seq, o.lane);
		} else if (strncmp(sample_seq, "input#", 6) == 0) {   /* what :1973-1975 do: four digits, plus 1, a 1-based sheet line */
			int line = 1;
			for (int k = 0, w = 1000; k < 4; k++, w /= 10) line += (sample_seq[6 + k] - '0') * w;
			sample_no = (int)(HashTableGet(cct_context->lineno1B_to_sampleno1B_tab, NULL + line) - NULL);
		}
		o.sample = sample_no;
		memcpy(o.bc, BC_seq, bl);
		memcpy(o.umi, UMI_seq, ul);
		fwrite(&o, sizeof o, 1, out);
		free(read_name);
	}
	for (int i = 0; i < n_pairs; i++) {
		char ab[66];
		if (fread(ab, 1, 66, fp) != 66) return 2;
		int32_t d[2] = {hamming_dist_ATGC_max1(ab, ab + 33), hamming_dist_ATGC_max1_2p(ab, ab + 33)};
		fwrite(d, 4, 2, out);
	}
	fclose(fp);
	fclose(out);
	return 0;
}
