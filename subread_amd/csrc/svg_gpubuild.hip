// svg_gpubuild.hip -- build a Subread index directly in HBM, with the reference's block structure.
//
// Same index as svg_build.c / subread-buildindex (index-builder.c:78-684,
// sorted-hashtable.c:1689-1908), built with HBM passes instead of the reference's per-bucket
// insertion + selection sort.  Once for the genome:
//   1. k_count        every sampled 16-mer (genekey2int packing) bumps a 2^32-entry
//                     occurrence counter (scan_gene_index's repeat scan)
//      k_kept         one kept bit per window (key seen <= threshold times) + kept counts per
//                     1024-window tile, prefix-summed; the 16 GiB of counters are freed here
//      plan           svg_blockplan.h: where build_gene_index closes its blocks (one block when
//                     force_one_block is set or no split point is reached), answered from the
//                     tile prefix and the bits of single tiles
// then for every block, over its window range [w_lo, w_hi] and into a handle of its own:
//   2. k_hist         kept windows bump their bucket (key % nb; nb is the same for all blocks)
//   3. exclusive scan of the bucket histogram -> bucket start offsets
//   4. k_scatter      kept windows land in their bucket (unordered)
//   5. k_sort         each bucket is sorted by (key_hi, then position ascending if
//                     (key % 791) is even, else descending) -- is_1_greater_than_2; a total
//                     order, so the scatter's atomic order does not show
// The blocks are then assembled as svg_index_open does (block 0 holds blocks 1.., stored = 1).
// The result is identical item-for-item to the CPU builder (tests check the written files against
// the reference md5s).  HBM peak: 16 GiB counters + genome + 1 bit/window; afterwards genome +
// 10 B/item per block; a 3 Gbp genome builds in seconds.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "svg_device.h"

#define PAD 1210

__device__ __forceinline__ uint32_t gb2i(char c) { return c < 'G' ? (c == 'A' ? 0u : 2u) : (c == 'G' ? 1u : 3u); }

struct WinMap {
	const char *bases;
	const uint64_t *gstart;   // contig start in bases
	const uint64_t *lin;      // linear coordinate of the contig's first base (O_c)
	const uint64_t *wcum;     // windows before contig c (n_ctg+1)
	uint32_t nctg;
	uint64_t nwin;
	int gap;
};

__device__ __forceinline__ void win_at(const WinMap &m, uint64_t w, uint32_t *key, uint32_t *pos)
{
	uint32_t lo = 0, hi = m.nctg - 1;
	while (lo < hi) { uint32_t mid = (lo + hi + 1) >> 1; if (m.wcum[mid] <= w) lo = mid; else hi = mid - 1; }
	uint64_t t = w - m.wcum[lo];
	const char *b = m.bases + m.gstart[lo] + t * (uint64_t)m.gap;
	uint32_t k = 0;
#pragma unroll
	for (int i = 0; i < 16; i++) k |= gb2i(b[i]) << (30 - 2 * i);
	*key = k;
	*pos = (uint32_t)(m.lin[lo] + t * (uint64_t)m.gap);
}

__global__ void k_count(WinMap m, uint32_t *cnt)
{
	for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w < m.nwin; w += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t key, pos;
		win_at(m, w, &key, &pos);
		atomicAdd(&cnt[key], 1u);
	}
}

// One kept bit per window (cnt[key] <= thr) and the kept count of every tile of KEPT_TILE windows:
// after this pass the 2^32 counters are no longer needed.  A wave's 64 consecutive windows make one
// 64-bit word (ballot), written by its first lane; blockDim.x must be 256.  bits holds
// ntiles * KEPT_TILE / 64 words (the last tile is padded with zero bits).
#define KEPT_TILE 1024
#define KEPT_WORDS (KEPT_TILE / 64)

__global__ void __launch_bounds__(256) k_kept(WinMap m, const uint32_t *cnt, uint32_t thr, uint64_t *bits, uint32_t *tcnt, uint32_t ntiles)
{
	__shared__ uint32_t s_n[4];
	const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
	for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
		uint32_t n = 0;
		for (int it = 0; it < KEPT_TILE / 256; it++) {
			const uint64_t w = (uint64_t)tile * KEPT_TILE + (uint64_t)it * 256 + threadIdx.x;
			bool kept = false;
			if (w < m.nwin) {
				uint32_t key, pos;
				win_at(m, w, &key, &pos);
				kept = cnt[key] <= thr;
			}
			const uint64_t b = __ballot(kept);
			if (lane == 0) {
				bits[w >> 6] = b;
				n += (uint32_t)__popcll(b);
			}
		}
		if (lane == 0) s_n[wv] = n;
		__syncthreads();
		if (threadIdx.x == 0) tcnt[tile] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
		__syncthreads();
	}
}

__device__ __forceinline__ bool kept_bit(const uint64_t *bits, uint64_t w) { return (bits[w >> 6] >> (w & 63)) & 1; }

// passes 2 and 4 over one block's windows [w_lo, w_lo + n)
__global__ void k_hist(WinMap m, const uint64_t *bits, uint64_t w_lo, uint64_t n, uint32_t nb, uint32_t *bcnt)
{
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t key, pos;
		if (!kept_bit(bits, w_lo + i)) continue;
		win_at(m, w_lo + i, &key, &pos);
		atomicAdd(&bcnt[key % nb], 1u);
	}
}

__global__ void k_scatter(WinMap m, const uint64_t *bits, uint64_t w_lo, uint64_t n, uint32_t nb, const uint32_t *bstart,
                          uint32_t *cursor, int16_t *keys, uint32_t *vals)
{
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t key, pos;
		if (!kept_bit(bits, w_lo + i)) continue;
		win_at(m, w_lo + i, &key, &pos);
		uint32_t b = key % nb;
		uint32_t slot = bstart[b] + atomicAdd(&cursor[b], 1u);
		keys[slot] = (int16_t)(key / nb);
		vals[slot] = pos;
	}
}

__device__ __forceinline__ uint64_t sort_key(int16_t kh, uint32_t pos, uint32_t b, uint32_t nb)
{
	uint32_t real = (uint32_t)kh * nb + b;   // is_1_greater_than_2: real_key = k1*all_buckets + bucket
	uint32_t pa = ((real % 791) % 2 == 0) ? pos : ~pos;
	return ((uint64_t)(uint16_t)kh << 32) | pa;
}

__global__ void k_sort(const uint32_t *bstart, uint32_t nb, int16_t *keys, uint32_t *vals)
{
	for (uint64_t bb = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; bb < nb; bb += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t b = (uint32_t)bb, s = bstart[b], e = bstart[b + 1];
		for (uint32_t i = s + 1; i < e; i++) {
			int16_t kh = keys[i];
			uint32_t v = vals[i];
			uint64_t sk = sort_key(kh, v, b, nb);
			uint32_t j = i;
			while (j > s && sort_key(keys[j - 1], vals[j - 1], b, nb) > sk) {
				keys[j] = keys[j - 1];
				vals[j] = vals[j - 1];
				j--;
			}
			keys[j] = kh;
			vals[j] = v;
		}
	}
}

static int grid_for(uint64_t n) { uint64_t g = (n + 255) / 256; return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g)); }

#define GCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { svg_set_error("HIP error %s at %s:%d", hipGetErrorString(_e), __FILE__, __LINE__); rc = SVG_E_DEVICE; goto fail; } } while (0)

// The block planner's view of the repeat scan (svg_blockplan.h): the tile prefix on the host, the
// bitmap in HBM; a question costs one binary search and the download of one or two tiles' bits.
struct KeptView {
	const uint64_t *d_bits;
	const uint32_t *pref;   // kept windows before tile t, [ntiles + 1]
	uint32_t ntiles;
	uint64_t nwin;
};

// kept windows among [0, w), w <= nwin
static int kept_rank(const KeptView *v, uint64_t w, uint64_t *out)
{
	const uint64_t tile = w / KEPT_TILE, in = w % KEPT_TILE;
	uint64_t n = v->pref[tile], bits[KEPT_WORDS];
	if (in) {
		HIPCHK(hipMemcpy(bits, v->d_bits + tile * KEPT_WORDS, sizeof bits, hipMemcpyDeviceToHost));
		for (uint64_t k = 0; k < in / 64; k++) n += (uint64_t)__builtin_popcountll(bits[k]);
		if (in % 64) n += (uint64_t)__builtin_popcountll(bits[in / 64] & ((1ull << (in % 64)) - 1));
	}
	*out = n;
	return 0;
}

static int kept_reach(void *ctx, uint64_t w0, uint64_t budget, uint64_t *w)
{
	const KeptView *v = (const KeptView *)ctx;
	uint64_t r0, bits[KEPT_WORDS];
	int rc = kept_rank(v, w0, &r0);
	if (rc) return rc;
	if (!budget) { *w = w0; return 1; }
	if (budget > (uint64_t)v->pref[v->ntiles] - r0) return 0;
	const uint64_t k = r0 + budget - 1;   // the window wanted is the k-th kept one of the genome (0-based)
	uint32_t lo = 0, hi = v->ntiles - 1;  // the last tile with pref[tile] <= k holds it
	while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (v->pref[mid] <= k) lo = mid; else hi = mid - 1; }
	HIPCHK(hipMemcpy(bits, v->d_bits + (uint64_t)lo * KEPT_WORDS, sizeof bits, hipMemcpyDeviceToHost));
	uint64_t left = k - v->pref[lo];
	for (int q = 0; q < KEPT_WORDS; q++) {
		const uint64_t c = (uint64_t)__builtin_popcountll(bits[q]);
		if (left < c) {
			uint64_t x = bits[q];
			while (left--) x &= x - 1;
			*w = (uint64_t)lo * KEPT_TILE + 64 * (uint64_t)q + (uint64_t)__builtin_ctzll(x);
			return 1;
		}
		left -= c;
	}
	svg_set_error("kept bitmap and its tile counts disagree (tile %u)", lo);
	return SVG_E_DEVICE;
}

static int kept_count(void *ctx, uint64_t w_lo, uint64_t w_hi, uint64_t *n)
{
	const KeptView *v = (const KeptView *)ctx;
	uint64_t a, b;
	int rc = kept_rank(v, w_lo, &a);
	if (!rc) rc = kept_rank(v, w_hi + 1, &b);
	if (!rc) *n = b - a;
	return rc;
}

// passes 2-5 for the windows of one block, into h's own d_bstart / d_keys / d_vals
// (d_bcnt: nb + 1 words, doubles as the scatter cursor; *d_tmp: hipcub's scratch, grown on demand)
static int build_block_device(svg_index *h, const WinMap &m, const uint64_t *d_bits, const svg_bp_block *B, uint32_t nb,
                              uint32_t *d_bcnt, void **d_tmp, size_t *tmp_cap)
{
	const uint64_t nw = B->w_hi - B->w_lo + 1;
	size_t need = 0;
	uint32_t tot = 0;
	int rc;
	if (B->items > 0xffffffffull) { svg_set_error("more than 2^32-1 items"); return SVG_E_UNSUPPORTED; }
	HIPCHK(hipMemset(d_bcnt, 0, 4 * ((size_t)nb + 1)));
	hipLaunchKernelGGL(k_hist, dim3(grid_for(nw)), dim3(256), 0, 0, m, d_bits, B->w_lo, nw, nb, d_bcnt);
	HIPCHK(hipGetLastError());
	if ((rc = dmalloc(h, &h->d_bstart, 4 * ((size_t)nb + 1)))) return rc;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(NULL, need, d_bcnt, (uint32_t *)h->d_bstart, (int)nb + 1));
	if (need + 16 > *tmp_cap) {
		hipFree(*d_tmp);
		*d_tmp = NULL;
		*tmp_cap = 0;
		HIPCHK(hipMalloc(d_tmp, need + 16));
		*tmp_cap = need + 16;
	}
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(*d_tmp, need, d_bcnt, (uint32_t *)h->d_bstart, (int)nb + 1));
	HIPCHK(hipMemcpy(&tot, (uint32_t *)h->d_bstart + nb, 4, hipMemcpyDeviceToHost));
	if (tot != B->items) { svg_set_error("block holds %u items, its plan %llu", tot, (unsigned long long)B->items); return SVG_E_DEVICE; }
	if ((rc = dmalloc(h, &h->d_keys, 2 * (size_t)tot + 64)) || (rc = dmalloc(h, &h->d_vals, 4 * (size_t)tot + 64))) return rc;
	HIPCHK(hipMemset(d_bcnt, 0, 4 * ((size_t)nb + 1)));
	hipLaunchKernelGGL(k_scatter, dim3(grid_for(nw)), dim3(256), 0, 0, m, d_bits, B->w_lo, nw, nb, (const uint32_t *)h->d_bstart,
	                   d_bcnt, (int16_t *)h->d_keys, (uint32_t *)h->d_vals);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_sort, dim3(grid_for(nb)), dim3(256), 0, 0, (const uint32_t *)h->d_bstart, nb, (int16_t *)h->d_keys,
	                   (uint32_t *)h->d_vals);
	HIPCHK(hipGetLastError());
	HIPCHK(hipDeviceSynchronize());
	h->host.items = tot;
	return 0;
}

// host side of one block's handle, as svg_host.c's loader leaves it for <prefix>.NN.b.*: the
// block's .array image, the genome-wide chromosome table
static int build_block_host(svg_index *h, const svg_genome *g, const uint64_t *O, const svg_blockplan *P, uint32_t k, uint32_t nb, int gap)
{
	const svg_bp_block *B = &P->blk[k];
	svg_host_index *x = &h->host;
	x->nb = nb; x->gap = gap; x->padding = PAD;
	x->start_point = (uint32_t)B->start;
	x->start_base_offset = x->start_point - x->start_point % 4;
	x->values = svg_pack_array_block(g, O, B->start, B->last_set, P->seg + B->s0, B->ns, &x->length, &x->values_bytes);
	x->n_chr = g->nctg;
	x->chr_end = (uint32_t *)malloc(4 * (size_t)g->nctg);
	x->chr_name = (char (*)[200])malloc(200 * (size_t)g->nctg);
	if (!x->values || !x->chr_end || !x->chr_name) { svg_set_error("out of host memory packing .array"); return SVG_E_NOMEM; }
	for (uint32_t c = 0; c < g->nctg; c++) {
		x->chr_end[c] = (uint32_t)(O[c] + g->ctg[c].len - 16 + PAD);
		memcpy(x->chr_name[c], g->ctg[c].name, 200);
	}
	return 0;
}

// <prefix>.NN.b.tab / .NN.b.array of one built block
static int save_block(const svg_index *h, const char *prefix, int block)
{
	const svg_host_index *x = &h->host;
	uint32_t *hb = (uint32_t *)malloc(4 * ((size_t)x->nb + 1));
	int16_t *hk = (int16_t *)malloc(2 * x->items + 2);
	uint32_t *hv = (uint32_t *)malloc(4 * x->items + 4);
	int rc = 0;
	if (!hb || !hk || !hv) { rc = SVG_E_NOMEM; svg_set_error("out of host memory saving index"); }
	if (!rc && (hipMemcpy(hb, h->d_bstart, 4 * ((size_t)x->nb + 1), hipMemcpyDeviceToHost) != hipSuccess ||
	            hipMemcpy(hk, h->d_keys, 2 * x->items, hipMemcpyDeviceToHost) != hipSuccess ||
	            hipMemcpy(hv, h->d_vals, 4 * x->items, hipMemcpyDeviceToHost) != hipSuccess)) {
		rc = SVG_E_DEVICE;
		svg_set_error("download of index block %d failed", block);
	}
	if (!rc) rc = svg_write_tab_block(prefix, block, x->nb, x->items, x->gap, hb, hk, hv);
	free(hb); free(hk); free(hv);
	if (!rc) rc = svg_write_array_block(prefix, block, x->start_point, x->length, x->values, x->values_bytes);
	return rc;
}

static int build_from_genome(svg_genome *g, int gap, int memory_mb, int force_one_block, int thr, int device,
                             const char *save_prefix, const char *source, svg_index **out)
{
	int rc = 0;
	uint64_t nwin = 0, kept_total = 0;
	uint64_t *O = NULL, *wcum = NULL, *gst = NULL;
	uint32_t *clen = NULL, *pref = NULL;
	char *d_bases = NULL;
	uint64_t *d_gst = NULL, *d_lin = NULL, *d_wcum = NULL, *d_bits = NULL;
	uint32_t *d_cnt = NULL, *d_bcnt = NULL, *d_tcnt = NULL, *d_pref = NULL;
	void *d_tmp = NULL;
	size_t tmp_cap = 0;
	svg_index *hb[SVG_MAX_BLOCKS] = {NULL};
	svg_blockplan plan = {NULL, NULL, 0, 0, 0, 0};
	uint32_t nb, ntiles;
	uint64_t budget;
	WinMap m;
	*out = NULL;
	if (gap != 1 && gap != 3) { svg_set_error("gap must be 1 or 3"); return SVG_E_ARG; }
	if (thr < 1) thr = 100;
	{
		int ndev = 0;
		if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { svg_set_error("no HIP device visible"); return SVG_E_DEVICE; }
		if (device < 0 || device >= ndev) { svg_set_error("device %d out of range", device); return SVG_E_ARG; }
	}
	if (hipSetDevice(device) != hipSuccess) { svg_set_error("hipSetDevice failed"); return SVG_E_DEVICE; }
	O = (uint64_t *)malloc(sizeof(uint64_t) * g->nctg);
	wcum = (uint64_t *)malloc(sizeof(uint64_t) * (g->nctg + 1));
	gst = (uint64_t *)malloc(sizeof(uint64_t) * g->nctg);
	clen = (uint32_t *)malloc(sizeof(uint32_t) * g->nctg);
	svg_genome_layout(g, gap, O, &nwin);
	if (O[g->nctg - 1] + g->ctg[g->nctg - 1].len + PAD >= 0xffffffffull) { free(O); free(wcum); free(gst); free(clen); svg_set_error("genome too long for 32-bit coordinates"); return SVG_E_UNSUPPORTED; }
	wcum[0] = 0;
	for (uint32_t c = 0; c < g->nctg; c++) {
		wcum[c + 1] = wcum[c] + (g->ctg[c].len - 16) / gap + 1;
		gst[c] = g->ctg[c].start;
		clen[c] = g->ctg[c].len;
	}
	budget = svg_items_budget(gap, memory_mb, force_one_block);
	nb = svg_bucket_count(budget, gap);
	ntiles = (uint32_t)((nwin + KEPT_TILE - 1) / KEPT_TILE);   // nwin < 2^32: positions are 32-bit

	GCHK(hipMalloc(&d_bases, g->nbases + 64));
	GCHK(hipMalloc(&d_gst, 8 * (size_t)g->nctg));
	GCHK(hipMalloc(&d_lin, 8 * (size_t)g->nctg));
	GCHK(hipMalloc(&d_wcum, 8 * ((size_t)g->nctg + 1)));
	GCHK(hipMemcpy(d_bases, g->bases, g->nbases, hipMemcpyHostToDevice));
	GCHK(hipMemcpy(d_gst, gst, 8 * (size_t)g->nctg, hipMemcpyHostToDevice));
	GCHK(hipMemcpy(d_lin, O, 8 * (size_t)g->nctg, hipMemcpyHostToDevice));
	GCHK(hipMemcpy(d_wcum, wcum, 8 * ((size_t)g->nctg + 1), hipMemcpyHostToDevice));
	m.bases = d_bases; m.gstart = d_gst; m.lin = d_lin; m.wcum = d_wcum; m.nctg = g->nctg; m.nwin = nwin; m.gap = gap;

	// 1. the genome-wide repeat scan, folded into one kept bit per window
	GCHK(hipMalloc(&d_cnt, sizeof(uint32_t) << 32));
	GCHK(hipMemset(d_cnt, 0, sizeof(uint32_t) << 32));
	hipLaunchKernelGGL(k_count, dim3(grid_for(nwin)), dim3(256), 0, 0, m, d_cnt);
	GCHK(hipGetLastError());
	GCHK(hipMalloc(&d_bits, 8 * (size_t)ntiles * KEPT_WORDS));
	GCHK(hipMalloc(&d_tcnt, 4 * ((size_t)ntiles + 1)));
	GCHK(hipMalloc(&d_pref, 4 * ((size_t)ntiles + 1)));
	GCHK(hipMemset(d_tcnt, 0, 4 * ((size_t)ntiles + 1)));
	hipLaunchKernelGGL(k_kept, dim3(ntiles > 65536 ? 65536 : ntiles), dim3(256), 0, 0, m, (const uint32_t *)d_cnt, (uint32_t)thr,
	                   d_bits, d_tcnt, ntiles);
	GCHK(hipGetLastError());
	GCHK(hipDeviceSynchronize());
	hipFree(d_cnt); d_cnt = NULL;
	{
		size_t need = 0;
		GCHK(hipcub::DeviceScan::ExclusiveSum(NULL, need, d_tcnt, d_pref, (int)ntiles + 1));
		GCHK(hipMalloc(&d_tmp, need + 16));
		tmp_cap = need + 16;
		GCHK(hipcub::DeviceScan::ExclusiveSum(d_tmp, need, d_tcnt, d_pref, (int)ntiles + 1));
		pref = (uint32_t *)malloc(4 * ((size_t)ntiles + 1));
		if (!pref) { rc = SVG_E_NOMEM; svg_set_error("out of host memory"); goto fail; }
		GCHK(hipMemcpy(pref, d_pref, 4 * ((size_t)ntiles + 1), hipMemcpyDeviceToHost));
		kept_total = pref[ntiles];
	}

	// the block plan: one block when forced (no window ever reaches the budget), else the reference's splits
	{
		KeptView view = {d_bits, pref, ntiles, nwin};
		svg_bp_kept K = {&view, kept_reach, kept_count};
		rc = svg_blockplan_make(O, clen, g->nctg, gap, force_one_block ? UINT64_MAX : budget, SVG_MAX_BLOCKS, &K, &plan);
		if (rc == SVG_BP_E_WALK) { rc = SVG_E_UNSUPPORTED; svg_set_error("more than 100 index blocks: raise memory_mb"); }
		else if (rc == SVG_BP_E_LIMIT) { rc = SVG_E_UNSUPPORTED; svg_set_error("more than %d index blocks (the most a handle holds): raise memory_mb", SVG_MAX_BLOCKS); }
		else if (rc == SVG_BP_E_NOMEM) { rc = SVG_E_NOMEM; svg_set_error("out of host memory planning the blocks"); }
		if (rc) goto fail;
	}

	// 2-5. every block's table, each into a handle of its own
	GCHK(hipMalloc(&d_bcnt, 4 * ((size_t)nb + 1)));
	for (uint32_t k = 0; k < plan.nblk; k++) {
		if (!(hb[k] = (svg_index *)calloc(1, sizeof(svg_index)))) { rc = SVG_E_NOMEM; svg_set_error("out of memory"); goto fail; }
		hb[k]->device = device;
		if ((rc = build_block_device(hb[k], m, d_bits, &plan.blk[k], nb, d_bcnt, &d_tmp, &tmp_cap))) goto fail;
	}
	hipFree(d_bases); d_bases = NULL;
	hipFree(d_gst); d_gst = NULL;
	hipFree(d_lin); d_lin = NULL;
	hipFree(d_wcum); d_wcum = NULL;
	hipFree(d_bits); d_bits = NULL;
	hipFree(d_tcnt); d_tcnt = NULL;
	hipFree(d_pref); d_pref = NULL;
	hipFree(d_bcnt); d_bcnt = NULL;
	hipFree(d_tmp); d_tmp = NULL;

	for (uint32_t k = 0; k < plan.nblk; k++) {
		if ((rc = build_block_host(hb[k], g, O, &plan, k, nb, gap))) goto fail;
		if (save_prefix && (rc = save_block(hb[k], save_prefix, (int)k))) goto fail;
	}
	if (save_prefix) {
		svg_unlink_blocks_from(save_prefix, (int)plan.nblk);
		if ((rc = svg_write_reads_files(save_prefix, g, O, gap, nwin, kept_total, nb, (int)plan.nblk, source))) goto fail;
	}
	// the handle, as svg_index_open assembles it: block 0 holds the others, voted after it in order
	for (uint32_t k = 0; k < plan.nblk; k++)
		if ((rc = svg_index_finish_device(hb[k]))) goto fail;
	for (uint32_t k = 1; k < plan.nblk; k++) {
		hb[0]->blk[k] = hb[k];
		hb[k]->stored = 1;
		hb[0]->device_bytes += hb[k]->device_bytes;
	}
	hb[0]->nblocks = (int)plan.nblk;
	svg_blockplan_free(&plan);
	free(O); free(wcum); free(gst); free(clen); free(pref);
	*out = hb[0];
	return 0;
fail:
	hipFree(d_bases); hipFree(d_gst); hipFree(d_lin); hipFree(d_wcum);
	hipFree(d_cnt); hipFree(d_bits); hipFree(d_tcnt); hipFree(d_pref); hipFree(d_bcnt); hipFree(d_tmp);
	free(O); free(wcum); free(gst); free(clen); free(pref);
	svg_blockplan_free(&plan);
	for (int k = 0; k < SVG_MAX_BLOCKS; k++)
		if (hb[k]) svg_index_close(hb[k]);   // not linked yet: each closes alone
	return rc;
}

extern "C" int svg_index_build(const char *fasta, int gap, int memory_mb, int force_one_block, int repeat_threshold,
                               int device, const char *save_prefix, svg_index **out)
{
	svg_genome g;
	int rc;
	if (!fasta || !out) { svg_set_error("svg_index_build: NULL argument"); return SVG_E_ARG; }
	memset(&g, 0, sizeof g);
	rc = svg_genome_read_fasta(fasta, &g);
	if (!rc) rc = build_from_genome(&g, gap, memory_mb, force_one_block, repeat_threshold, device, save_prefix, fasta, out);
	svg_genome_free(&g);
	return rc;
}

extern "C" int svg_index_build_mem(const char *const *names, const char *const *seqs, const uint64_t *lens, uint32_t n_ctg,
                                   int gap, int memory_mb, int force_one_block, int repeat_threshold, int device,
                                   const char *save_prefix, svg_index **out)
{
	svg_genome g;
	int rc;
	if (!names || !seqs || !lens || !out) { svg_set_error("svg_index_build_mem: NULL argument"); return SVG_E_ARG; }
	rc = svg_genome_from_mem(names, seqs, lens, n_ctg, &g);
	if (!rc) rc = build_from_genome(&g, gap, memory_mb, force_one_block, repeat_threshold, device, save_prefix, "<memory>", out);
	svg_genome_free(&g);
	return rc;
}
