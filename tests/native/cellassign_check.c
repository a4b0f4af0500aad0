/* TEST INFRASTRUCTURE ONLY: a program of its own over the host builder
 * (subread_amd/csrc/svg_cell_annot.c) and cellassign_model.c, built with
 * -fsanitize=address,undefined by tests/test_cellassign_model.py; no Python process and no GPU
 * takes part in its run.  It draws seeded annotations (equal starts, features across a bucket
 * border, a contig without features), records and barcodes, and compares
 *   - the model's gene lists with a scan of every feature of the contig in table order (the block
 *     and reverse-table walk may skip only what cannot overlap),
 *   - the model's barcode numbers with a scan of the whole whitelist in the reference's order
 *     (exact, else the first of the F-row entries, then of the other S-row entries, at distance 1).
 *
 *   cellassign_check [seed]      exit status 0: equal */
#include "../../subread_amd/csrc/svg_cell_annot.c"
#include "cellassign_model.c"

static uint64_t rs;
static uint32_t rnd(uint32_t n) { rs = rs * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((rs >> 33) % n); }

static int check_genes(uint64_t seed)
{
	rs = seed;
	enum { NC = 4, NF = 3000, NR = 4000 };
	const int padding = 1210;
	const uint32_t len[NC] = {400000, 5000, 300000, 2000};   /* contig 1 gets no feature */
	uint32_t chr_end[NC], at = 0;
	for (int c = 0; c < NC; c++) { at += len[c] + 2 * padding - 16; chr_end[c] = at; }
	svg_cell_feature *f = calloc(NF, sizeof *f);
	for (int i = 0; i < NF; i++) {
		const int c = (int[]){0, 2, 3}[rnd(3)];
		f[i].contig = (uint32_t)c;
		f[i].start = i % 5 == 0 && i ? f[i - 1].start : 1 + rnd(len[c]);   /* equal starts */
		if (i % 97 == 0 && c != 3) f[i].start = 131072 - 50 + rnd(40);    /* across the bucket border */
		f[i].end = f[i].start + 20 + rnd(400);
		f[i].gene = (int32_t)rnd(400);
		f[i].is_negative_strand = (uint8_t)rnd(2);
		if (i % 5 == 0 && i) f[i].contig = f[i - 1].contig;
	}
	svg_cell_annot a;
	char why[256];
	if (svg_cell_annot_build(f, NF, chr_end, NC, padding, &a, why, sizeof why)) { fprintf(stderr, "%s\n", why); return 1; }
	svg_cell_aln *r = calloc(NR, sizeof *r);
	for (int i = 0; i < NR; i++) {
		r[i].position = rnd(at + 3000);
		r[i].flags = (int16_t)(rnd(2) * 16);
		const char *forms[] = {"%dM", "%dS%dM", "%dM%dS", "%dM2D%dM", "%dM3I%dM", "%dM50N%dM1D%dM"};
		snprintf(r[i].cigar, sizeof r[i].cigar, forms[rnd(6)], 5 + rnd(60), 5 + rnd(120), 5 + rnd(200));
	}
	svg_cell_hit *hits = calloc(NR, sizeof *hits);
	int32_t *genes = malloc(4 * (size_t)NR * 512);
	int bad = 0;
	for (int allow = 0; allow < 2; allow++) {
		const int64_t ng = cellassign_model(&a, allow, 0, chr_end, NC, padding, r, NR, hits, genes, (uint64_t)NR * 512);
		if (ng < 0) { fprintf(stderr, "gene list over its bound\n"); return 1; }
		for (int i = 0; i < NR && !bad; i++) {
			if (hits[i].contig < 0) continue;
			/* the longest M from chro_pos covers every other: one scan of the contig's features */
			int longest = 0, v = 0;
			for (const char *p = r[i].cigar; *p; p++) {
				if (*p >= '0' && *p <= '9') v = v * 10 + (*p - '0');
				else { if (*p == 'M' && v > longest) longest = v; v = 0; }
			}
			const int64_t b = hits[i].chro_pos, e = b + longest;
			int32_t want[512];
			int nw = 0;
			for (uint32_t q = 0; q < a.n_features; q++) {
				/* the contig of item q: its block's */
				uint32_t c = 0, blk = 0;
				while (a.block_end[blk] <= q) blk++;
				while (a.chro_block_end[c] <= blk) c++;
				if ((int)c != hits[i].contig || a.end[q] < b || a.start[q] > e || a.strand[q] != ((r[i].flags & 16) ? 1 : 0)) continue;
				int k = 0;
				while (k < nw && want[k] != a.gene[q]) k++;
				if (k == nw && nw < 512) want[nw++] = a.gene[q];
			}
			if (nw > 1 && !allow) nw = 0;
			if ((uint32_t)nw != hits[i].nhits || memcmp(want, genes + hits[i].first_gene, 4 * (size_t)nw)) {
				fprintf(stderr, "record %d (allow %d): %d genes by the full scan, %u by the model\n", i, allow, nw, hits[i].nhits);
				bad = 1;
			}
		}
	}
	svg_cell_annot_free(&a);
	free(f); free(r); free(hits); free(genes);
	return bad;
}

static int check_barcodes(uint64_t seed, int L)
{
	rs = seed + (uint64_t)L;
	enum { NB = 3000 };
	const int NW = L < 5 ? (1 << (2 * L)) / 2 : 600;   /* distinct barcodes of L bases */
	const char acgt[] = "ACGT";
	char *wl = calloc((size_t)NW, (size_t)L + 1), *rd = calloc(NB, (size_t)L + 1);
	int nw = 0;
	while (nw < NW) {
		char *s = wl + (size_t)nw * (L + 1);
		if (nw && rnd(3)) { memcpy(s, wl + (size_t)rnd((uint32_t)nw) * (L + 1), (size_t)L); for (uint32_t k = 1 + rnd(2); k; k--) s[rnd((uint32_t)L)] = acgt[rnd(4)]; }
		else for (int k = 0; k < L; k++) s[k] = acgt[rnd(4)];
		int dup = 0;
		for (int j = 0; j < nw && !dup; j++) dup = !memcmp(wl + (size_t)j * (L + 1), s, (size_t)L);
		if (!dup) nw++;
	}
	for (int i = 0; i < NB; i++) {
		char *s = rd + (size_t)i * (L + 1);
		memcpy(s, wl + (size_t)rnd((uint32_t)NW) * (L + 1), (size_t)L);
		for (uint32_t k = rnd(4); k; k--) s[rnd((uint32_t)L)] = rnd(5) ? acgt[rnd(4)] : 'N';
	}
	int32_t *got = malloc(4 * NB);
	if (cellassign_model_barcodes(wl, (uint64_t)NW, L, rd, NB, got)) return 1;
	int bad = 0;
	for (int i = 0; i < NB && !bad; i++) {
		const char *s = rd + (size_t)i * (L + 1);
		int want = -1;
		for (int j = 0; j < NW && want < 0; j++) if (!memcmp(wl + (size_t)j * (L + 1), s, (size_t)L)) want = j;
		for (int pass = 0; pass < 2 && want < 0; pass++)   /* F-row entries first, then S-row entries */
			for (int j = 0; j < NW && want < 0; j++) {
				const char *w = wl + (size_t)j * (L + 1);
				int same_half = 1, mism = 0;
				for (int k = 0; k < L / 2; k++) same_half &= w[2 * k + pass] == s[2 * k + pass];
				for (int k = 0; k < L; k++) mism += w[k] != s[k];
				if (same_half && mism == 1) want = j;
			}
		if (want != got[i]) { fprintf(stderr, "barcode %d (%s, length %d): %d by the full scan, %d by the model\n", i, s, L, want, got[i]); bad = 1; }
	}
	free(wl); free(rd); free(got);
	return bad;
}

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], NULL, 10) : 1;
	int bad = check_genes(seed);
	for (int L = 2; L <= 16 && !bad; L++) bad = check_barcodes(seed, L);
	printf("%s\n", bad ? "DIFFERENT" : "equal");
	return bad;
}
