/* Stand-alone check of tests/native/cellname_model.c under the address and undefined-behaviour
 * sanitizers (tests/test_cellname_model.py builds and runs it; no Python, no GPU): random names in both
 * modes, well-formed and damaged, through the model and through a restatement that first cuts the
 * name at its separators and then compares index texts position by position; and the tallies against
 * a call-by-call count.  Exit status 0 and "cellname_check OK" when they agree everywhere. */
#include <stdio.h>
#include "cellname_model.c"

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 11) % n; }

static int atgcn(int c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; }

/* the restatement: separator positions first */
static void brute(const char *nm, int len, int bcl, int bl, int ul, const cellname_sheet *sh, int32_t out[5], char *bc, char *umi)
{
	int sep[5], ns = 0;
	for (int i = 1; i < len && ns < 5; i++)
		if (nm[i] == '|' || (bcl && nm[i] == ':')) sep[ns++] = i;
	out[0] = ns; out[1] = ns ? sep[0] : 0; out[2] = -1; out[3] = -1; out[4] = 0;
	memset(bc, 'A', bl); memset(umi, 'A', ul);
	if (ns < 3) { out[4] = 1; return; }
	if (sep[0] + 1 + bl + ul > len) { out[4] = 2; return; }
	for (int k = 0; k < bl + ul; k++) if (!atgcn(nm[sep[0] + 1 + k])) { out[4] = 3; return; }
	memcpy(bc, nm + sep[0] + 1, bl); memcpy(umi, nm + sep[0] + 1 + bl, ul);
	const int s3 = sep[2] + 1;
	if (ns == 5) {
		int lp = sep[4] + 1;
		if (lp + 9 <= len && !memcmp(nm + lp, "@RgLater@", 9)) lp += 9;
		unsigned no = 0;
		for (int i = lp + 1; i < len && nm[i] >= '0' && nm[i] <= '9'; i++) no = no * 10u + (unsigned)(nm[i] - '0');
		out[2] = (int)no;
		int run = 0;
		while (s3 + run < len && atgcn(nm[s3 + run])) run++;
		for (int x = 0; x < sh->n_rows; x++) {
			if (sh->row_lane[x] != LANE_ALL && sh->row_lane[x] != out[2]) continue;
			const char *known = sh->row_text + (size_t)x * ROW_BYTES;
			const int kl = (int)strlen(known), sl = run < kl ? run : kl;
			int first = 0, second = 0, all = 0;
			for (int k = 0; k < sl; k++)
				if (nm[s3 + k] != known[k]) { all++; if (k < sl / 2) first++; else second++; }
			if (kl > 12 ? (first <= 1 && second <= 1) : all <= 1) { out[3] = sh->row_sample[x]; break; }
		}
	} else if (s3 + 6 <= len && !memcmp(nm + s3, "input#", 6)) {
		int line = 1;
		for (int k = 0, w = 1000; k < 4; k++, w /= 10) line += ((s3 + 6 + k < len ? nm[s3 + 6 + k] : 0) - '0') * w;
		out[3] = line >= 1 && line <= sh->n_lines ? sh->lines[line - 1] : 0;
	}
}

int main(void)
{
	const int32_t row_lane[6] = {LANE_ALL, LANE_ALL, 2, LANE_ALL, LANE_ALL, 3}, row_sample[6] = {1, 2, 3, 4, 5, 6};
	const char *texts[6] = {"ACGTACGT", "ACGTACGA", "TTGGCCAA", "TTGGCCAT", "GATTACAGCTTACAGA", "GGGGGGGGTTTTTTTTGGGGGGGGTTTTTTTT"};
	char row_text[6 * ROW_BYTES];
	memset(row_text, 0, sizeof row_text);
	for (int i = 0; i < 6; i++) strcpy(row_text + i * ROW_BYTES, texts[i]);
	const int32_t lines[5] = {1, 0, 6, 0, 3};
	const cellname_sheet sh = {6, 5, row_lane, row_sample, row_text, lines};
	long checked = 0;
	for (int it = 0; it < 60000; it++) {
		const int bcl = it & 1, bl = 1 + (int)rnd(16), ul = 1 + (int)rnd(14);
		char nm[400];
		int len = 0;
		len += sprintf(nm + len, "R%011d%c", it, bcl && rnd(8) ? ':' : '|');
		for (int k = 0; k < bl + ul; k++) nm[len++] = "ACGTN"[rnd(5)];
		if (rnd(30) == 0) nm[13 + rnd(bl + ul)] = "!acgt|"[rnd(6)];
		nm[len++] = '|';
		for (int k = 0; k < bl + ul; k++) nm[len++] = "#-.0125<ACFGHIJK"[rnd(16)];
		if (rnd(6) == 0) nm[len - 1 - rnd(bl + ul)] = ':';
		nm[len++] = '|';
		if (rnd(5) == 0) len += sprintf(nm + len, "input#%04d@L%03d", (int)rnd(8), 1 + (int)rnd(4));
		else {
			const char *t = texts[rnd(6)];
			int tl = (int)strlen(t);
			if (rnd(4) == 0) tl -= 1 + (int)rnd(3);
			for (int k = 0; k < tl; k++) nm[len++] = rnd(10) == 0 ? "ACGTN"[rnd(5)] : t[k];
			for (int k = (int)rnd(4); rnd(4) == 0 && k > 0; k--) nm[len++] = "ACGT"[rnd(4)];
			nm[len++] = '|';
			for (int k = 0; k < tl; k++) nm[len++] = 'F';
			if (rnd(8)) len += sprintf(nm + len, rnd(6) ? "|@RgLater@L%03d" : "|L%d", 1 + (int)rnd(4));
		}
		if (rnd(25) == 0) len = (int)rnd((uint32_t)len + 1);          /* cut anywhere, to nothing as well */
		char *heap = malloc(len ? len : 1);                          /* no byte behind the name belongs to it */
		memcpy(heap, nm, len);
		int32_t a[5], b[5];
		char abc[16], aum[16], bbc[16], bum[16];
		cellname_parse(heap, len, bcl, bl, ul, &sh, a, abc, aum);
		brute(heap, len, bcl, bl, ul, &sh, b, bbc, bum);
		if (memcmp(a, b, sizeof a) || memcmp(abc, bbc, bl) || memcmp(aum, bum, ul)) {
			printf("MISMATCH %.*s (bcl %d bl %d ul %d): model %d %d %d %d %d, brute %d %d %d %d %d\n", len, heap, bcl, bl, ul, a[0], a[1], a[2], a[3],
			       a[4], b[0], b[1], b[2], b[3], b[4]);
			return 1;
		}
		free(heap);
		checked++;
	}
	/* the tallies, call by call: a record with contig -1 is an unmapped call (this_multi_mapping_i 0) */
	enum { N = 5000, S = 3 };
	static uint32_t nrec[N], nhits[N], status[N];
	static int32_t contig[N], sample[N];
	uint64_t want[3 * (S + 1)] = {0}, got[3 * (S + 1)];
	for (int i = 0; i < N; i++) {
		nrec[i] = rnd(4); contig[i] = (int32_t)rnd(3) - 1; nhits[i] = rnd(3); sample[i] = (int32_t)rnd(S + 3) - 1; status[i] = rnd(20) == 0;
		if (status[i] || sample[i] > S) continue;
		const int calls = nrec[i] ? (int)nrec[i] : 1;
		for (int cidx = 0; cidx < calls; cidx++) {
			const int reporting_index = nrec[i] && !(cidx == 0 && contig[i] < 0) ? 0 : -1, this_i = cidx + 1;
			const int hits = cidx == 0 ? (int)nhits[i] : 0;
			if (sample[i] > 0) {
				want[sample[i] - 1]++;
				if (cidx == 0 && reporting_index >= 0 && this_i == 1) { want[S + 1 + sample[i] - 1]++; if (hits > 0) want[2 * (S + 1) + sample[i] - 1]++; }
			} else want[S]++;
		}
	}
	cellname_tallies(N, nrec, contig, nhits, sample, status, S, got);
	if (memcmp(want, got, sizeof want)) { printf("MISMATCH in the tallies\n"); return 1; }
	printf("cellname_check OK: %ld names\n", checked);
	return 0;
}
