/* TEST INFRASTRUCTURE ONLY: a program of its own that runs cellalign_model.c over one case written
 * by tests/cellalign_common.py write_case (16 u64: buckets, gap, items, values_bytes,
 * start_base_offset, exons, sequence bytes, reads, expected records, the 7 parameters; then bstart,
 * keys, vals, values, exon starts, exon stops, the reads' text, offsets and lengths, the expected
 * heads and records) and compares every byte.  Built with -fsanitize=address,undefined by
 * tests/test_cellalign_golden.py; no Python process and no GPU takes part in its run.
 *
 *   cellalign_check <case.bin>      exit status 0: equal */
#include "cellalign_model.c"

static void *take(FILE *f, size_t bytes)
{
	void *p = malloc(bytes ? bytes : 1);
	if (!p || fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "short case file\n"); exit(2); }
	return p;
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
	uint64_t *h = take(f, 16 * 8);
	const uint64_t nb = h[0], items = h[2], vbytes = h[3], sbo = h[4], nex = h[5], nseq = h[6], n = h[7], nexp = h[8];
	aparams_t p = {(int32_t)h[9], (int32_t)h[10], (int32_t)h[11], (int32_t)h[12], (int32_t)h[13], (int32_t)h[14], (int32_t)h[15]};
	uint32_t *bstart = take(f, 4 * (nb + 1));
	int16_t *keys = take(f, 2 * items);
	uint32_t *vals = take(f, 4 * items);
	uint8_t *values = take(f, vbytes);
	uint32_t *ea = take(f, 4 * nex), *eb = take(f, 4 * nex);
	char *seq = take(f, nseq);
	uint64_t *off = take(f, 8 * n);
	uint16_t *len = take(f, 2 * n);
	ahead_t *want_h = take(f, sizeof(ahead_t) * n);
	aln_t *want_a = take(f, sizeof(aln_t) * nexp);
	fclose(f);
	uint64_t bits = sbo + 4 * vbytes + EXON_TAIL;
	if (bits > (1ull << 32)) bits = 1ull << 32;
	bits = (bits + 31) / 32 * 32;
	uint8_t *planes = nex ? malloc(bits / 8 * 2) : NULL;
	if (nex) cellalign_model_planes(ea, eb, nex, planes, bits);
	ahead_t *heads = calloc(n ? n : 1, sizeof *heads);
	aln_t *alns = calloc((n ? n : 1) * (size_t)p.max_reported_alignments_per_read, sizeof *alns);
	const int64_t k = cellalign_model((uint32_t)nb, (int)h[1], bstart, keys, vals, values, (uint32_t)vbytes, (uint32_t)sbo, planes,
	                                  nex ? bits : 0, seq, off, len, n, &p, heads, alns, NULL, NULL);
	int bad = k != (int64_t)nexp || memcmp(heads, want_h, sizeof(ahead_t) * n) || memcmp(alns, want_a, sizeof(aln_t) * nexp);
	printf("%llu reads, %lld records: %s\n", (unsigned long long)n, (long long)k, bad ? "DIFFERENT" : "equal");
	free(h); free(bstart); free(keys); free(vals); free(values); free(ea); free(eb); free(seq); free(off); free(len);
	free(want_h); free(want_a); free(planes); free(heads); free(alns);
	return bad;
}
