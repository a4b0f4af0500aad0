/* TEST INFRASTRUCTURE ONLY: a program of its own over cellumi_model.c, built with
 * -fsanitize=address,undefined by tests/test_cellumi_model.py; no Python process and no GPU takes
 * part in its run.  It draws seeded observations (short UMIs over a small alphabet, so that
 * sections of 1 .. several hundred entries, merges and chains occur; sections of 29 .. 33 entries
 * on purpose) and compares the model with a brute-force restatement over text UMIs:
 *   - supports by counting equal observations, O(n^2);
 *   - step 1 with the reference's own data structure, keyed lists ('F' + first half, 'S' + second
 *     half, cell-counts.c:3566-3634) searched by key text, or one list (:3598-3620);
 *   - step 2 without a sort: a survivor counts if every other survivor of its (cell, UMI) has a
 *     strictly smaller support; it is the removed one if it is the first by (support descending,
 *     gene) and does not count;
 *   - the count table by scanning.
 *
 *   cellumi_check [seed]      exit status 0: equal */
#include <stdio.h>
#include "cellumi_model.c"

static uint64_t rs;
static uint32_t rnd(uint32_t n) { rs = rs * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((rs >> 33) % n); }

typedef struct { char key[SVG_CELL_MAX_UMI + 2]; uint32_t n; uint32_t *item; } keyed_list;

static int before1(const svg_cell_umi_entry *l, const svg_cell_umi_entry *r, int L)
{
	if (l->sample != r->sample) return l->sample < r->sample;
	if (l->cell != r->cell) return l->cell < r->cell;
	if (l->gene != r->gene) return l->gene < r->gene;
	if (l->support != r->support) return l->support > r->support;
	return memcmp(l->umi, r->umi, (size_t)L) < 0;
}

static int brute(const int32_t *sample, const int32_t *cell, const int64_t *gene, const char *umi, uint32_t n, int L, int n_samples,
                 svg_cell_umi_entry *e, uint64_t *n_entries, svg_cell_count *counts, uint64_t *n_counts, uint64_t *removed)
{
	uint32_t ne = 0;
	memset(removed, 0, 8 * (size_t)n_samples);
	for (uint32_t i = 0; i < n; i++) {
		if (sample[i] <= 0 || cell[i] < 0) continue;
		uint32_t k = 0;
		for (; k < ne; k++)
			if (e[k].sample == sample[i] && e[k].cell == cell[i] && e[k].gene == gene[i] && !memcmp(e[k].umi, umi + (size_t)i * L, (size_t)L)) break;
		if (k < ne) { e[k].support++; continue; }
		memset(&e[ne], 0, sizeof e[ne]);
		e[ne].sample = sample[i]; e[ne].cell = cell[i]; e[ne].gene = (int32_t)gene[i]; e[ne].support = 1;
		memcpy(e[ne].umi, umi + (size_t)i * L, (size_t)L);
		ne++;
	}
	for (uint32_t i = 1; i < ne; i++) {          /* insertion sort into step 1's order */
		svg_cell_umi_entry t = e[i];
		uint32_t j = i;
		while (j && before1(&t, &e[j - 1], L)) { e[j] = e[j - 1]; j--; }
		e[j] = t;
	}
	for (uint32_t i = 0; i < ne; i++) { e[i].support_merged = e[i].support; e[i].outcome = SVG_CELL_UMI_LOST; }
	keyed_list *tab = calloc(2 * (size_t)ne + 2, sizeof *tab);
	uint32_t *one = malloc(4 * ((size_t)ne + 1));
	if (!tab || !one) return 1;
	const int half = L / 2;
	for (uint32_t a = 0; a < ne;) {
		uint32_t b = a + 1;
		while (b < ne && e[b].sample == e[a].sample && e[b].cell == e[a].cell && e[b].gene == e[a].gene) b++;
		const int look = b - a > 30;
		uint32_t ntab = 0, none = 0;
		for (uint32_t i = a; i < b; i++) {
			int found = 0;
			char key[2][SVG_CELL_MAX_UMI + 2];
			for (int hx = 0; hx < 2; hx++) {
				memset(key[hx], 0, sizeof key[hx]);
				key[hx][0] = hx ? 'S' : 'F';
				memcpy(key[hx] + 1, e[i].umi + hx * L / 2, (size_t)half);
			}
			for (int hx = 0; hx < (look ? 2 : 1) && !found; hx++) {
				const uint32_t *items = one;
				uint32_t cnt = none;
				if (look) {
					cnt = 0;
					for (uint32_t t = 0; t < ntab; t++)
						if (!strcmp(tab[t].key, key[hx])) { items = tab[t].item; cnt = tab[t].n; }
				}
				for (uint32_t x = 0; x < cnt && !found; x++) {
					svg_cell_umi_entry *q = e + items[x];
					int d = 0;
					for (int c = 0; c < L; c++) d += q->umi[c] != e[i].umi[c];
					if (d < 2) {
						found = 1;
						q->support_merged += e[i].support;
						e[i].outcome = SVG_CELL_UMI_MERGED;
						memcpy(e[i].acceptor_umi, q->umi, (size_t)L);
					}
				}
			}
			if (found) continue;
			if (!look) { one[none++] = i; continue; }
			for (int hx = 0; hx < 2; hx++) {
				uint32_t t = 0;
				while (t < ntab && strcmp(tab[t].key, key[hx])) t++;
				if (t == ntab) { strcpy(tab[t].key, key[hx]); tab[t].n = 0; tab[t].item = malloc(4 * (size_t)(b - a)); if (!tab[t].item) return 1; ntab++; }
				tab[t].item[tab[t].n++] = i;
			}
		}
		for (uint32_t t = 0; t < ntab; t++) free(tab[t].item);
		a = b;
	}
	free(tab); free(one);
	for (uint32_t i = 0; i < ne; i++) {
		if (e[i].outcome == SVG_CELL_UMI_MERGED) continue;
		int counts_ = 1, first = 1;
		for (uint32_t j = 0; j < ne; j++) {
			if (j == i || e[j].outcome == SVG_CELL_UMI_MERGED || e[j].sample != e[i].sample || e[j].cell != e[i].cell ||
			    memcmp(e[j].umi, e[i].umi, (size_t)L)) continue;
			if (e[j].support_merged >= e[i].support_merged) counts_ = 0;
			if (e[j].support_merged > e[i].support_merged || (e[j].support_merged == e[i].support_merged && e[j].gene < e[i].gene)) first = 0;
		}
		if (counts_) e[i].outcome = SVG_CELL_UMI_COUNTED;
		else if (first) { e[i].outcome = SVG_CELL_UMI_REMOVED; removed[e[i].sample - 1]++; }
	}
	uint64_t nc = 0;
	for (uint32_t i = 0; i < ne; i++) {
		if (e[i].outcome != SVG_CELL_UMI_COUNTED) continue;
		uint64_t k = 0;
		while (k < nc && (counts[k].sample != e[i].sample || counts[k].cell != e[i].cell || counts[k].gene != e[i].gene)) k++;
		if (k == nc) { counts[nc].sample = e[i].sample; counts[nc].cell = e[i].cell; counts[nc].gene = e[i].gene; counts[nc].n_umis = 0; nc++; }
		counts[k].n_umis++;
	}
	*n_entries = ne;
	*n_counts = nc;
	return 0;
}

/* one run: `cells` x `genes` sections over UMIs of length L from the first `alpha` letters of ACGTN */
static int run(uint64_t seed, uint32_t n, int L, uint32_t alpha, uint32_t cells, uint32_t genes, uint32_t forced_section)
{
	rs = seed;
	enum { S = 2 };
	int32_t *sample = malloc(4 * (size_t)n), *cell = malloc(4 * (size_t)n);
	int64_t *gene = malloc(8 * (size_t)n);
	char *umi = malloc((size_t)n * (size_t)L);
	svg_cell_umi_entry *e1 = malloc(sizeof *e1 * n), *e2 = malloc(sizeof *e2 * n);
	svg_cell_count *c1 = malloc(sizeof *c1 * n), *c2 = malloc(sizeof *c2 * n);
	if (!sample || !cell || !gene || !umi || !e1 || !e2 || !c1 || !c2) return 1;
	for (uint32_t i = 0; i < n; i++) {
		sample[i] = (int32_t)rnd(S + 1);                     /* 0: no sample */
		cell[i] = (int32_t)rnd(cells + 1) - 1;               /* -1: no cell */
		gene[i] = rnd(genes) * 1000003ll % 0x7fffffffll;
		if (i < forced_section) { sample[i] = 1; cell[i] = 0; gene[i] = 5; }
		for (int k = 0; k < L; k++) umi[(size_t)i * L + k] = "ACGTN"[rnd(alpha)];
		if (i && rnd(3) == 0) {                                /* a near copy of an earlier observation: supports above 1, chains */
			const uint32_t j = rnd(i);
			sample[i] = sample[j]; cell[i] = cell[j]; gene[i] = rnd(2) ? gene[j] : gene[i];
			memcpy(umi + (size_t)i * L, umi + (size_t)j * L, (size_t)L);
			if (rnd(2)) umi[(size_t)i * L + rnd((uint32_t)L)] = "ACGTN"[rnd(alpha)];
		}
	}
	uint64_t ne1, ne2, nc1, nc2, rem1[S], rem2[S], dropped[2];
	if (cellumi_model(sample, cell, gene, umi, n, L, S, 0, e1, &ne1, c1, &nc1, rem1, dropped)) { fprintf(stderr, "model failed\n"); return 1; }
	if (brute(sample, cell, gene, umi, n, L, S, e2, &ne2, c2, &nc2, rem2)) return 1;
	int bad = 0;
	if (ne1 != ne2 || nc1 != nc2 || memcmp(rem1, rem2, sizeof rem1)) bad = 1;
	if (!bad && memcmp(e1, e2, sizeof *e1 * ne1)) bad = 2;
	for (uint64_t i = 0; i < nc1 && !bad; i++) {             /* the brute table is in first-seen order */
		uint64_t k = 0;
		while (k < nc2 && memcmp(&c1[i], &c2[k], sizeof c1[i])) k++;
		if (k == nc2) bad = 3;
	}
	if (bad) fprintf(stderr, "seed %llu n %u L %d alpha %u: model and brute force differ (%d): entries %llu/%llu counts %llu/%llu\n",
	                 (unsigned long long)seed, n, L, alpha, bad, (unsigned long long)ne1, (unsigned long long)ne2, (unsigned long long)nc1, (unsigned long long)nc2);
	uint32_t merged = 0;
	for (uint64_t i = 0; i < ne1; i++) merged += e1[i].outcome == SVG_CELL_UMI_MERGED;
	printf("n %u L %d alpha %u: entries %llu merged %u counts %llu removed %llu+%llu\n", n, L, alpha, (unsigned long long)ne1, merged,
	       (unsigned long long)nc1, (unsigned long long)rem1[0], (unsigned long long)rem1[1]);
	free(sample); free(cell); free(gene); free(umi); free(e1); free(e2); free(c1); free(c2);
	return bad;
}

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], NULL, 10) : 1;
	int bad = 0;
	for (int L = 1; L <= SVG_CELL_MAX_UMI && !bad; L++) bad |= run(seed + (uint64_t)L, 3000, L, L < 4 ? 5 : 2 + (uint32_t)(L % 3), 3, 4, 0);
	for (uint32_t sz = 25; sz <= 70 && !bad; sz++) bad |= run(seed * 31 + sz, sz + 40, 6 + (int)(sz % 3), 3, 2, 2, sz);
	if (!bad) bad |= run(seed + 99, 6000, 11, 2, 1, 2, 2500);
	if (!bad) bad |= run(seed + 100, 6000, 12, 5, 2, 3, 0);
	return bad ? 1 : 0;
}
