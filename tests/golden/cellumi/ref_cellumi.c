/* Driver over the REFERENCE's UMI stage, used by make_cellumi_golden.py only.  It #includes the
 * reference's cell-counts.c where it lies (-DREF_CELL_COUNTS=...; nothing of it is copied here) and
 * puts observations through the reference's own code, in the order of cellCounts_do_one_batch
 * (cell-counts.c:3991-4071): ADD_key_struct, cellCounts_do_one_batch_tab_to_struct_list, ArrayListSort
 * with cellCounts_do_one_batch_tab_to_struct_list_compare and both calls of
 * cellCounts_do_one_batch_UMI_merge_one_step.
 *
 *   ref-cellumi in.bin out_prefix
 * in.bin: int32 L, S, n; int32 sample[n]; int32 cell[n]; int64 gene[n]; char umi[n][L].  An
 * observation whose sample is below 1 is left out (the reference's list index would be -1, :3774).
 * Per sample s (1-based) it writes
 *   <prefix>.s<s>.entries  one record per struct in the order after the first sort: the struct as
 *                          sorted (cell, gene, UMI, supp_reads), cellbc and supp_reads after step
 *                          1, the index of the acceptor read from filtered_CGU_table (-1: not
 *                          merged; -2: its key, which holds no cell (:3581-3587), was taken by
 *                          another cell's entry), the struct's place in the list after the second
 *                          sort, and cellbc after step 2;
 *   <prefix>.s<s>.counts   int64 (cell, gene, UMIs) of the final table in iteration order;
 *   <prefix>.s<s>.removed  int64 removed_UMIs of this sample. */
#define main cellcounts_unused_main
#include REF_CELL_COUNTS
#undef main

#pragma pack(push, 1)
typedef struct {
	int32_t cell0; int64_t gene; char umi[MAX_UMI_LEN]; int32_t supp0;
	int32_t cell1, supp1, acceptor, rank2, cell2;
} dump_rec;
#pragma pack(pop)

typedef struct { char *key; void *val; } kv;
static kv *g_kv;
static srInt_64 g_nkv;
static void collect_kv(void *k, void *v, HashTable *t) { g_kv[g_nkv].key = k; g_kv[g_nkv].val = v; g_nkv++; }

typedef struct { void *p; int idx; } pidx;
static int pidx_cmp(const void *a, const void *b) { const pidx *l = a, *r = b; return l->p < r->p ? -1 : l->p > r->p; }
static int find_idx(pidx *tab, int n, void *p)
{
	pidx k = {p, 0}, *f = bsearch(&k, tab, n, sizeof *tab, pidx_cmp);
	return f ? f->idx : -2;
}

static FILE *g_counts;
static void dump_count(void *k, void *v, HashTable *t)
{
	srInt_64 key = (k - NULL) - 1, rec[3] = {key >> 32, key & 0xffffffffll, v - NULL};
	fwrite(rec, 8, 3, g_counts);
}

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	FILE *fp = fopen(argv[1], "rb");
	int hdr[3];
	if (!fp || fread(hdr, 4, 3, fp) != 3) return 2;
	const int L = hdr[0], S = hdr[1], n = hdr[2];
	int *sample = malloc(4 * (size_t)n + 4), *cell = malloc(4 * (size_t)n + 4);
	srInt_64 *gene = malloc(8 * (size_t)n + 8);
	char *umi = malloc((size_t)n * L + 1);
	if (fread(sample, 4, n, fp) != n || fread(cell, 4, n, fp) != n || fread(gene, 8, n, fp) != n || fread(umi, L, n, fp) != n) return 2;
	fclose(fp);
	cellcounts_global_t *cct_context = calloc(1, sizeof *cct_context);
	cct_context->UMI_length = L;

	HashTable *supp_reads_SCGU = StringTableCreate(500000);
	HashTableSetDeallocationFunctions(supp_reads_SCGU, free, NULL);
	char UMI_str[MAX_UMI_LEN + 1];
	for (int i = 0; i < n; i++) {
		int sample_id = sample[i], cell_no = cell[i];
		srInt_64 gene_no = gene[i];
		if (sample_id < 1) continue;
		memcpy(UMI_str, umi + (size_t)i * L, L);
		UMI_str[L] = 0;
		ADD_key_struct;
	}
	ArrayList **cell_gene_umi_list = malloc(sizeof(void *) * S);
	srInt_64 x1;
	for (x1 = 0; x1 < S; x1++) {
		cell_gene_umi_list[x1] = ArrayListCreate(2000000);
		ArrayListSetDeallocationFunction(cell_gene_umi_list[x1], free);
	}
	supp_reads_SCGU->appendix1 = cell_gene_umi_list;
	supp_reads_SCGU->appendix2 = cct_context;
	supp_reads_SCGU->counter1 = L;
	HashTableIteration(supp_reads_SCGU, cellCounts_do_one_batch_tab_to_struct_list);
	HashTable *filtered_SCGU_table = StringTableCreate(10000);
	HashTableSetDeallocationFunctions(filtered_SCGU_table, free, NULL);

	for (x1 = 0; x1 < S; x1++) {
		ArrayList *list = cell_gene_umi_list[x1];
		HashTable *cellbcP0_to_geneno0B_P1_to_UMIs = HashTableCreate(500000);
		void *app1[4];                      /* (:3526 reads app1[3], the sample number) */
		list->appendix1 = app1;
		app1[0] = cct_context;
		app1[1] = NULL + 1;
		app1[2] = NULL;
		app1[3] = NULL + (x1 + 1);
		ArrayListSort(list, cellCounts_do_one_batch_tab_to_struct_list_compare);
		const int ne = (int)list->numOfElements;
		dump_rec *rec = calloc(ne + 1, sizeof *rec);
		pidx *ptab = malloc(sizeof *ptab * (ne + 1));
		for (int i = 0; i < ne; i++) {
			struct cell_gene_umi_supp *s = ArrayListGet(list, i);
			rec[i].cell0 = s->cellbc; rec[i].gene = s->gene_no; rec[i].supp0 = s->supp_reads;
			memcpy(rec[i].umi, s->umi, L);
			ptab[i].p = s; ptab[i].idx = i;
		}
		qsort(ptab, ne, sizeof *ptab, pidx_cmp);
		const srInt_64 keys_before = filtered_SCGU_table->numOfElements;
		cellCounts_do_one_batch_UMI_merge_one_step(list, 0, filtered_SCGU_table, NULL);
		g_kv = malloc(sizeof *g_kv * (filtered_SCGU_table->numOfElements + 1));
		g_nkv = 0;
		HashTableIteration(filtered_SCGU_table, collect_kv);
		for (int i = 0; i < ne; i++) {
			struct cell_gene_umi_supp *s = ArrayListGet(list, i);
			rec[i].cell1 = s->cellbc; rec[i].supp1 = s->supp_reads;
			rec[i].acceptor = -1;
			if (rec[i].cell0 < 0 || s->cellbc >= 0) continue;
			char key[60 + MAX_UMI_LEN];
			int kp = SUBreadSprintf(key, sizeof key, "%d-%d-%lld-", (int)(x1 + 1), -1, (long long)s->gene_no);
			memcpy(key + kp, s->umi, L);
			key[kp + L] = 0;
			rec[i].acceptor = -2;
			for (srInt_64 q = 0; q < g_nkv; q++) {
				if (strcmp(g_kv[q].key, key)) continue;
				const int a = find_idx(ptab, ne, (char *)g_kv[q].val - offsetof(struct cell_gene_umi_supp, umi));
				if (a >= 0 && rec[a].cell0 == rec[i].cell0 && rec[a].gene == rec[i].gene) rec[i].acceptor = a;
			}
		}
		free(g_kv);
		(void)keys_before;

		app1[1] = NULL + 0;
		app1[2] = cellbcP0_to_geneno0B_P1_to_UMIs;
		ArrayListSort(list, cellCounts_do_one_batch_tab_to_struct_list_compare);
		int *rank_of = malloc(4 * (ne + 1));
		for (int i = 0; i < ne; i++) rank_of[i] = find_idx(ptab, ne, ArrayListGet(list, i));
		srInt_64 removed_UMIs = 0;
		cellCounts_do_one_batch_UMI_merge_one_step(list, 1, filtered_SCGU_table, &removed_UMIs);
		for (int i = 0; i < ne; i++) {
			struct cell_gene_umi_supp *s = ArrayListGet(list, i);
			rec[rank_of[i]].rank2 = i;
			rec[rank_of[i]].cell2 = s->cellbc;
		}
		char name[4096];
		snprintf(name, sizeof name, "%s.s%d.entries", argv[2], (int)(x1 + 1));
		fp = fopen(name, "wb"); fwrite(rec, sizeof *rec, ne, fp); fclose(fp);
		snprintf(name, sizeof name, "%s.s%d.counts", argv[2], (int)(x1 + 1));
		g_counts = fopen(name, "wb");
		HashTableIteration(cellbcP0_to_geneno0B_P1_to_UMIs, dump_count);
		fclose(g_counts);
		snprintf(name, sizeof name, "%s.s%d.removed", argv[2], (int)(x1 + 1));
		fp = fopen(name, "wb"); fwrite(&removed_UMIs, 8, 1, fp); fclose(fp);
		HashTableDestroy(cellbcP0_to_geneno0B_P1_to_UMIs);
		free(rec); free(ptab); free(rank_of);
	}
	return 0;
}
