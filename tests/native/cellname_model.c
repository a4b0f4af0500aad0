/* Plain-C model of svg_cell_parse_names and of svg_cell_counter_tallies (include/subread_vote.h): the
 * rules as the header states them, character by character on a NUL-terminated copy of the name, the
 * way cell-counts.c walks it.  tests/test_cellname_golden.py holds it to the reference's own answers
 * (tests/golden/cellname/), tests/native/cellname_check.c to a brute-force restatement under the
 * sanitizers, and the GPU tests hold the library to it.  tools/bench_cellnames.py times
 * cellname_parse_batch as what a caller pays on host threads without the device path. */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define LANE_ALL   99999
#define MAX_INDEX  32
#define ROW_BYTES  (MAX_INDEX + 1)
#define NAME_PAD   48            /* NUL bytes behind the copy: "@RgLater@", "input#NNNN" and an index are read past the end */

typedef struct {
	int n_rows, n_lines;
	const int32_t *row_lane, *row_sample;
	const char *row_text;        /* n_rows texts of ROW_BYTES bytes, NUL-padded */
	const int32_t *lines;
} cellname_sheet;

static int is_atgcn(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; }

/* hamming_dist_ATGC_max1 (input-blc.c:1094-1105) */
int cellname_max1(const char *a, const char *b)
{
	int x, same = 0;
	for (x = 0; is_atgcn(a[x]) && is_atgcn(b[x]); x++) {
		same += a[x] == b[x];
		if (x - same > 1) return 999;
	}
	return x - same;
}

/* hamming_dist_ATGC_max1_2p (input-blc.c:1072-1090) */
int cellname_max1_2p(const char *a, const char *b)
{
	int sl = 0, x, p1 = 0, p2 = 0;
	while (is_atgcn(a[sl]) && is_atgcn(b[sl])) sl++;
	sl /= 2;
	for (x = 0; is_atgcn(a[x]) && is_atgcn(b[x]); x++)
		if (a[x] != b[x]) { if (x < sl) p1++; else p2++; }
	return p1 > 1 || p2 > 1 ? 999 : p1 + p2;
}

/* cellCounts_get_sample_id (cell-counts.c:1862-1880) */
int cellname_sample_id(const cellname_sheet *sh, const char *sbc, int lane)
{
	for (int x = 0; x < sh->n_rows; x++) {
		if (sh->row_lane[x] != LANE_ALL && sh->row_lane[x] != lane) continue;
		const char *known = sh->row_text + (size_t)x * ROW_BYTES;
		if (strlen(known) > 12) { if (cellname_max1_2p(sbc, known) <= 2) return sh->row_sample[x]; }
		else if (cellname_max1(sbc, known) <= 1) return sh->row_sample[x];
	}
	return -1;
}

/* out: fields, trimmed length, lane, sample, status; bc and umi: bl and ul characters ('A' where refused) */
void cellname_parse(const char *name, int len, int bcl, int bl, int ul, const cellname_sheet *sh, int32_t out[5], char *bc, char *umi)
{
	char local[512 + NAME_PAD], *s = len <= 512 ? local : malloc((size_t)len + NAME_PAD);   /* (a name of the usual length costs no allocation) */
	memcpy(s, name, len);
	memset(s + len, 0, NAME_PAD);
	int field = 0, trimmed = 0, lane = -1, sample = -1, status = 0;
	char *bc_seq = NULL, *sample_seq = NULL, *lane_str = NULL;
	for (char *t = s + 1; len > 1 && *t; t++) {
		if (*t != '|' && !(*t == ':' && bcl)) continue;
		field++;
		if (field == 1) { trimmed = (int)(t - s); bc_seq = t + 1; }
		else if (field == 3) sample_seq = t + 1;
		else if (field == 5) {
			lane_str = t + 1;
			if (memcmp(lane_str, "@RgLater@", 9) == 0) lane_str += 9;
			break;
		}
	}
	memset(bc, 'A', bl);
	memset(umi, 'A', ul);
	if (field < 3) status = 1;
	else if ((bc_seq - s) + bl + ul > len) status = 2;
	else {
		for (int k = 0; k < bl + ul; k++)
			if (!is_atgcn(bc_seq[k])) status = 3;
		if (!status) { memcpy(bc, bc_seq, bl); memcpy(umi, bc_seq + bl, ul); }
	}
	if (!status && lane_str) {
		unsigned no = 0;
		for (char *t = lane_str + 1; *t >= '0' && *t <= '9'; t++) no = no * 10u + (unsigned)(*t - '0');
		lane = (int)no;
		sample = cellname_sample_id(sh, sample_seq, lane);
	} else if (!status && memcmp("input#", sample_seq, 6) == 0) {
		const int line = (sample_seq[6] - '0') * 1000 + (sample_seq[7] - '0') * 100 + (sample_seq[8] - '0') * 10 + (sample_seq[9] - '0') + 1;
		sample = line >= 1 && line <= sh->n_lines ? sh->lines[line - 1] : 0;
	}
	out[0] = field; out[1] = trimmed; out[2] = lane; out[3] = sample; out[4] = status;
	if (s != local) free(s);
}

/* bl (<= 16) characters as svg_packed_reads packs them: A 0, G 1, C 2, T 3; N: 3 and the exception bit */
static void pack16(const char *t, int n, uint32_t *bases, uint32_t *xmask)
{
	*bases = *xmask = 0;
	for (int k = 0; k < n; k++) {
		const uint32_t code = t[k] == 'A' ? 0u : t[k] == 'G' ? 1u : t[k] == 'C' ? 2u : 3u;
		*bases |= code << (30 - 2 * k);
		*xmask |= (uint32_t)(t[k] == 'N') << (31 - k);
	}
}

typedef struct {
	const char *text;
	const uint64_t *offs;
	const uint16_t *lens;
	uint64_t lo, hi;
	int bcl, bl, ul;
	const cellname_sheet *sh;
	int32_t *out;                /* [n][5] */
	uint32_t *packed;            /* [n][6]: barcode words 0 and 1, its exception word, the same of the UMI */
	char *bc, *umi;              /* [n][bl], [n][ul], or NULL */
} job;

static void *run(void *arg)
{
	job *j = arg;
	char b[16], u[16];
	for (uint64_t i = j->lo; i < j->hi; i++) {
		cellname_parse(j->text + j->offs[i], j->lens[i], j->bcl, j->bl, j->ul, j->sh, j->out + 5 * i, b, u);
		uint32_t *p = j->packed + 6 * i;
		pack16(b, j->bl, p, p + 2);
		pack16(u, j->ul, p + 3, p + 5);
		p[1] = p[4] = 0;
		if (j->bc) memcpy(j->bc + i * j->bl, b, j->bl);
		if (j->umi) memcpy(j->umi + i * j->ul, u, j->ul);
	}
	return NULL;
}

void cellname_parse_batch(const char *text, const uint64_t *offs, const uint16_t *lens, uint64_t n, int bcl, int bl, int ul, int n_rows,
                          const int32_t *row_lane, const int32_t *row_sample, const char *row_text, int n_lines, const int32_t *lines,
                          int32_t *out, uint32_t *packed, char *bc, char *umi, int threads)
{
	cellname_sheet sh = {n_rows, n_lines, row_lane, row_sample, row_text, lines};
	if (threads < 1) threads = 1;
	if (threads > 64) threads = 64;
	job jobs[64];
	pthread_t th[64];
	for (int t = 0; t < threads; t++) {
		job j = {text, offs, lens, n * t / threads, n * (t + 1) / threads, bcl, bl, ul, &sh, out, packed, bc, umi};
		jobs[t] = j;
		if (threads == 1) run(&jobs[t]);
		else pthread_create(&th[t], NULL, run, &jobs[t]);
	}
	for (int t = 0; t < threads && threads > 1; t++) pthread_join(th[t], NULL);
}

/* the tallies of cell-counts.c:1993-2004 as subread_vote.h states them: per read its number of records,
 * the contig and nhits of its first record (unused without records) and its sample number;
 * out: reads, mapped, assigned, S + 1 numbers each */
void cellname_tallies(uint64_t n, const uint32_t *n_records, const int32_t *first_contig, const uint32_t *first_nhits, const int32_t *sample,
                      const uint32_t *status, int S, uint64_t *out)
{
	memset(out, 0, 8 * 3 * ((size_t)S + 1));
	for (uint64_t i = 0; i < n; i++) {
		if ((status && status[i]) || sample[i] > S) continue;
		const uint64_t calls = n_records[i] ? n_records[i] : 1;
		if (sample[i] <= 0) { out[S] += calls; continue; }
		const int s = sample[i] - 1;
		out[s] += calls;
		if (n_records[i] && first_contig[i] >= 0) {
			out[S + 1 + s]++;
			if (first_nhits[i] > 0) out[2 * (S + 1) + s]++;
		}
	}
}
