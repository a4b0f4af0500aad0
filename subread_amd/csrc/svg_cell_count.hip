// svg_cell_count.hip -- cellCounts' UMI stage on the GPU: cellCounts_do_one_batch
// (cell-counts.c:3951-4126) from ADD_key_struct (:3945-3949) to the (cell, gene) -> UMIs table
// (:4068-4069), with cellCounts_do_one_batch_UMI_merge_one_step (:3644-3678) and
// cellCounts_do_one_batch_UMI_merge_one_cell (:3521-3642).  The contract is in
// include/subread_vote.h; the observations of svg_cell_count_batch come from svg_cell_assign.hip's
// chunk buffers while they are in device memory.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <hipcub/hipcub.hpp>
#include "svg_cell.h"
#include "svg_cell_umi.h"

#define U_NONE   0xffffffffu
#define U_SMALL  30                  // sec_end - sec_start > 30 takes the looktable rule (:3555)
#define U_LDS    2048                // accepted UMIs of a section that the wave kernel holds in LDS (24 KiB); the rest in HBM

struct svg_cell_counter {
	svg_index *h;
	int L, n_samples;
	uint64_t *d_hi, *d_lo;           // the observations: sample << 56 | cell << 32 | gene; the UMI code
	uint64_t cap;
	// observations, dropped_no_sample, dropped_no_cell, values outside their fields, refused read names; then
	// the tallies reads, mapped and assigned, n_samples + 1 each (:1993-2004)
	uint64_t *cnt;
	unsigned long long *d_cnt;       // the same on the device
	size_t cnt_bytes;
};

#define CNT_HEAD 5

struct ExpandParams {
	const svg_cell_aln_head *heads;  // the chunk's reads
	const svg_cell_hit *hits;        // the chunk's records
	const int32_t *genes;            // the chunk's gene lists
	const int32_t *bc;               // the chunk's barcode numbers, or NULL
	const int32_t *sample;           // the chunk's sample numbers
	const uint32_t *status;          // the chunk's name statuses (svg_cell_count_names_batch), or NULL
	const uint32_t *ubases, *uxmask;
	const uint64_t *ustarts;
	uint64_t ustride, ubase0, rec_base, gene_base, cap;
	uint32_t n, L;
	int n_samples;
	uint64_t *hi, *lo;
	unsigned long long *cnt;
};

// thread = read: one observation per (record, gene of its list) (:4011-4026)
__global__ void __launch_bounds__(256) count_expand_kernel(ExpandParams ep)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r >= ep.n) return;
	const svg_cell_aln_head hd = ep.heads[r];
	if (!hd.n_records) return;
	if (ep.status && ep.status[r]) return;        // a refused name: counted by count_tally_kernel
	const uint64_t j0 = hd.first_record - ep.rec_base;
	uint32_t total = 0;
	for (uint32_t j = 0; j < hd.n_records; j++) {
		const svg_cell_hit *h = ep.hits + j0 + j;
		if (h->contig >= 0) total += h->nhits;
	}
	if (!total) return;
	const int32_t sample = ep.sample[r], cell = ep.bc ? ep.bc[r] : -1;
	// as svg_cell_counter_add: a value outside its field is refused before anything is dropped
	uint32_t bad = sample > ep.n_samples || cell >= SVG_CELL_MAX_CELLS;
	for (uint32_t j = 0; j < hd.n_records && !bad; j++) {
		const svg_cell_hit *h = ep.hits + j0 + j;
		if (h->contig < 0) continue;
		for (uint32_t g = 0; g < h->nhits; g++)
			if (ep.genes[h->first_gene - ep.gene_base + g] < 0) bad = 1;
	}
	if (bad) { atomicAdd(ep.cnt + 3, (unsigned long long)total); return; }
	if (sample <= 0) { atomicAdd(ep.cnt + 1, (unsigned long long)total); return; }
	if (cell < 0) { atomicAdd(ep.cnt + 2, (unsigned long long)total); return; }
	const uint64_t ub = ep.ustarts ? ep.ustarts[r] : ep.ubase0 + (uint64_t)r * ep.ustride;
	uint64_t code = 0;
	for (uint32_t k = 0; k < ep.L; k++) {
		const uint64_t q = ub + k;
		const uint32_t b = (ep.ubases[q >> 4] >> (30u - 2u * (uint32_t)(q & 15u))) & 3u;
		const uint32_t x = ep.uxmask ? (ep.uxmask[q >> 5] >> (31u - (uint32_t)(q & 31u))) & 1u : 0u;
		code = code << 3 | umi_packed_code(b, x);
	}
	uint64_t at = atomicAdd(ep.cnt, (unsigned long long)total);
	if (at + total > ep.cap) return;      // (the host sized the store for the chunk's whole gene list: not reached)
	const uint64_t top = (uint64_t)sample << 56 | (uint64_t)cell << 32;
	for (uint32_t j = 0; j < hd.n_records; j++) {
		const svg_cell_hit *h = ep.hits + j0 + j;
		if (h->contig < 0) continue;
		for (uint32_t g = 0; g < h->nhits; g++) {
			ep.hi[at] = top | (uint32_t)ep.genes[h->first_gene - ep.gene_base + g];
			ep.lo[at] = code;
			at++;
		}
	}
}

// lane = read: the tallies of :1993-2004 over the calls of cellCounts_vote_and_add_count that the read's
// records stand for (subread_vote.h), and the refused names.  The lanes of a wave that share a
// sample slot are summed first: one atomic per wave, slot and tally
__global__ void __launch_bounds__(256) count_tally_kernel(ExpandParams ep)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	const bool live = r < ep.n;
	const int S = ep.n_samples;
	int slot = -1;
	uint32_t calls = 0;
	bool mapped = false, assigned = false, refused = false;
	if (live) {
		const svg_cell_aln_head hd = ep.heads[r];
		const int32_t sample = ep.sample[r];
		refused = ep.status && ep.status[r];
		if (!refused && sample <= S) {
			slot = sample > 0 ? sample - 1 : S;
			calls = hd.n_records ? hd.n_records : 1u;
			if (hd.n_records && sample > 0) {
				const svg_cell_hit *h = ep.hits + (hd.first_record - ep.rec_base);
				mapped = h->contig >= 0;
				assigned = mapped && h->nhits > 0;
			}
		}
	}
	const uint32_t lane = threadIdx.x & 63u;
	const unsigned long long nref = __ballot(refused);
	if (nref && lane == 0) atomicAdd(ep.cnt + 4, (unsigned long long)__popcll(nref));
	unsigned long long todo = __ballot(slot >= 0);
	while (todo) {
		const int s = __shfl(slot, __ffsll((long long)todo) - 1);
		const bool mine = slot == s;
		const unsigned long long same = __ballot(mine);
		uint32_t sum = mine ? calls : 0u;
		for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
		const uint32_t nm = (uint32_t)__popcll(__ballot(mine && mapped)), na = (uint32_t)__popcll(__ballot(mine && assigned));
		if (lane == 0) {
			unsigned long long *t = ep.cnt + CNT_HEAD;
			atomicAdd(t + s, (unsigned long long)sum);
			if (nm) atomicAdd(t + (S + 1) + s, (unsigned long long)nm);
			if (na) atomicAdd(t + 2 * (S + 1) + s, (unsigned long long)na);
		}
		todo &= ~same;
	}
}

struct FinishParams {
	uint32_t n, ne;                  // observations; entries
	const uint64_t *s_hi, *s_lo;     // the observations by (hi, lo)
	uint32_t *flag, *pos;            // head flags and their exclusive sum
	uint32_t *e_start;               // [ne + 1]
	uint64_t *e_hi0, *e_lo0;         // entries by (hi, UMI)
	uint32_t *supp0, *key_a, *idx;
	uint32_t *meta;                  // 0: entries, 1: sections, 2: big sections, 3: survivors, 4: rows of the count table
	// step 1's order
	uint64_t *e_hi, *e_lo;
	uint32_t *supp, *supp_after, *acceptor, *outcome, *counted;
	uint32_t *sec_start;             // [sections + 1]
	uint32_t *big;
	uint64_t *spill_code;            // the wave kernel's accepted lists past U_LDS, at the section's own entries
	uint32_t *spill_idx;
	uint64_t mask_f, mask_s;         // the two half keys of :3570
	// step 2's order
	const uint32_t *order;
	uint32_t n2;
	unsigned long long *removed;
};

__global__ void __launch_bounds__(256) obs_head_kernel(FinishParams fp)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= fp.n) return;
	fp.flag[i] = i == 0 || fp.s_hi[i] != fp.s_hi[i - 1] || fp.s_lo[i] != fp.s_lo[i - 1];
}

__global__ void __launch_bounds__(256) obs_start_kernel(FinishParams fp)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= fp.n) return;
	if (fp.flag[i]) fp.e_start[fp.pos[i]] = i;
	if (i == fp.n - 1) { const uint32_t ne = fp.pos[i] + fp.flag[i]; fp.e_start[ne] = fp.n; fp.meta[0] = ne; }
}

// thread = entry: its key and its support, the number of its observations (:3947-3949)
__global__ void __launch_bounds__(256) entry_kernel(FinishParams fp)
{
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;
	if (e >= fp.ne) return;
	const uint32_t a = fp.e_start[e], s = fp.e_start[e + 1] - a;
	fp.e_hi0[e] = fp.s_hi[a];
	fp.e_lo0[e] = fp.s_lo[a];
	fp.supp0[e] = s;
	fp.key_a[e] = ~s;
	fp.idx[e] = e;
}

__global__ void __launch_bounds__(256) gather_hi_kernel(const uint64_t *src, const uint32_t *idx, uint64_t *dst, uint32_t n)
{
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;
	if (e < n) dst[e] = src[idx[e]];
}

// the entries in step 1's order (:3725-3754 with sort_by_geneid_then_umi), and the section heads
__global__ void __launch_bounds__(256) order1_kernel(FinishParams fp, const uint32_t *idx)
{
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;
	if (e >= fp.ne) return;
	const uint32_t i = idx[e];
	fp.e_lo[e] = fp.e_lo0[i];
	fp.supp[e] = fp.supp_after[e] = fp.supp0[i];
	fp.acceptor[e] = U_NONE;
	fp.counted[e] = 0;
	fp.flag[e] = e == 0 || fp.e_hi[e] != fp.e_hi[e - 1];
}

__global__ void __launch_bounds__(256) section_kernel(FinishParams fp)
{
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;
	if (e >= fp.ne) return;
	if (fp.flag[e]) fp.sec_start[fp.pos[e]] = e;
	if (e == fp.ne - 1) { const uint32_t ns = fp.pos[e] + fp.flag[e]; fp.sec_start[ns] = fp.ne; fp.meta[1] = ns; }
}

// thread = (cell, gene) section of at most 30 entries: the list rule (:3598-3620).  The accepted
// list is the section's earlier entries that were not merged, in their order; larger sections go
// to step1_wave_kernel's list
__global__ void __launch_bounds__(256) step1_lane_kernel(FinishParams fp)
{
	const uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s >= fp.meta[1]) return;
	const uint32_t a = fp.sec_start[s], b = fp.sec_start[s + 1];
	if (b - a > (uint32_t)U_SMALL) { fp.big[atomicAdd(fp.meta + 2, 1u)] = s; return; }
	for (uint32_t i = a + 1; i < b; i++) {
		const uint64_t code = fp.e_lo[i];
		for (uint32_t j = a; j < i; j++) {
			if (fp.acceptor[j] != U_NONE) continue;
			if (umi_hamming(fp.e_lo[j], code) < 2) {
				fp.acceptor[i] = j;
				fp.supp_after[j] += fp.supp[i];
				break;
			}
		}
	}
}

// wave = section of more than 30 entries: the looktable rule (:3566-3597, :3622-3634).  The entries
// are walked in order; the accepted UMIs stand in acceptance order in LDS (the first U_LDS) and in
// HBM (the rest), the lanes test 64 of them at a time, and the list of a half key in the reference
// is that order restricted to the acceptors with the same half: the first near acceptor of the F
// list is the lowest set bit of the first ballot that has one, and only then of the S list
__global__ void __launch_bounds__(64) step1_wave_kernel(FinishParams fp)
{
	__shared__ uint64_t acode[U_LDS];
	__shared__ uint32_t aidx[U_LDS];
	const uint32_t lane = threadIdx.x, nbig = fp.meta[2];
	for (uint32_t bi = blockIdx.x; bi < nbig; bi += gridDim.x) {
		const uint32_t s = fp.big[bi], a = fp.sec_start[s], b = fp.sec_start[s + 1];
		uint32_t nacc = 0;
		for (uint32_t i = a; i < b; i++) {
			const uint64_t code = fp.e_lo[i];
			int found = -1;
			for (int hx = 0; hx < 2 && found < 0; hx++) {
				const uint64_t mask = hx ? fp.mask_s : fp.mask_f;
				for (uint32_t base = 0; base < nacc && found < 0; base += 64u) {
					const uint32_t k = base + lane;
					bool ok = false;
					if (k < nacc) {
						const uint64_t c = k < (uint32_t)U_LDS ? acode[k]
						                   : __hip_atomic_load(fp.spill_code + a + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						ok = ((c ^ code) & mask) == 0 && umi_hamming(c, code) < 2;
					}
					const unsigned long long bal = __ballot(ok);
					if (bal) found = (int)base + __ffsll((long long)bal) - 1;
				}
			}
			if (lane == 0) {
				if (found >= 0) {
					const uint32_t j = (uint32_t)found < (uint32_t)U_LDS ? aidx[found] : fp.spill_idx[a + (uint32_t)found];
					fp.acceptor[i] = j;
					fp.supp_after[j] += fp.supp[i];
				} else if (nacc < (uint32_t)U_LDS) {
					acode[nacc] = code;
					aidx[nacc] = i;
				} else {
					__hip_atomic_store(fp.spill_code + a + nacc, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					fp.spill_idx[a + nacc] = i;
					__threadfence();
				}
			}
			if (found < 0) nacc++;
			__syncthreads();
		}
	}
}

// thread = entry: merged or not; the survivors are selected into step 2's sort
__global__ void __launch_bounds__(256) survivor_kernel(FinishParams fp)
{
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;
	if (e >= fp.ne) return;
	const bool merged = fp.acceptor[e] != U_NONE;
	fp.flag[e] = !merged;
	fp.outcome[e] = merged ? SVG_CELL_UMI_MERGED : SVG_CELL_UMI_LOST;
}

// the three keys of step 2's order (:3725-3754 without sort_by_geneid_then_umi), least significant first
__global__ void __launch_bounds__(256) key2_kernel(FinishParams fp, const uint32_t *idx, uint64_t *k64, uint32_t *k32, int which)
{
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= fp.n2) return;
	const uint32_t i = idx[p];
	if (which == 0) k64[p] = (uint64_t)(~fp.supp_after[i]) << 32 | (uint32_t)fp.e_hi[i];
	else if (which == 1) k64[p] = fp.e_lo[i];
	else k32[p] = (uint32_t)(fp.e_hi[i] >> 32);
}

// thread = survivor in step 2's order: the head of a (cell, UMI) section looks at the entry behind it (:3528-3538, :3672)
__global__ void __launch_bounds__(256) step2_kernel(FinishParams fp)
{
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= fp.n2) return;
	const uint32_t i = fp.order[p];
	const uint32_t cell = (uint32_t)(fp.e_hi[i] >> 32);
	const uint64_t umi = fp.e_lo[i];
	if (p) {
		const uint32_t q = fp.order[p - 1];
		if ((uint32_t)(fp.e_hi[q] >> 32) == cell && fp.e_lo[q] == umi) return;      // not the first: dropped
	}
	bool counts = true;
	if (p + 1 < fp.n2) {
		const uint32_t q = fp.order[p + 1];
		if ((uint32_t)(fp.e_hi[q] >> 32) == cell && fp.e_lo[q] == umi) counts = fp.supp_after[i] > fp.supp_after[q];
	}
	if (counts) { fp.outcome[i] = SVG_CELL_UMI_COUNTED; fp.counted[i] = 1; }
	else { fp.outcome[i] = SVG_CELL_UMI_REMOVED; atomicAdd(fp.removed + (cell >> 24) - 1, 1ull); }
}

// ---------------------------------------------------------------------------------------------
// host side

static int counter_grow(svg_cell_counter *c, uint64_t need)
{
	if (need <= c->cap) return 0;
	svg_index *h = c->h;
	if (need >= (1ull << 31)) {
		svg_set_error("svg_cell_counter: %llu observations (a counter holds fewer than 2^31)", (unsigned long long)need);
		return SVG_E_UNSUPPORTED;
	}
	uint64_t cap = c->cap * 2 > need ? c->cap * 2 : need;
	if (cap < 4096) cap = 4096;
	const int64_t max_mb = svg_get_option("cell_count_max_mb");
	if (max_mb > 0 && cap * 16 > (uint64_t)max_mb << 20) cap = need;
	if (max_mb > 0 && cap * 16 > (uint64_t)max_mb << 20) {
		svg_set_error("svg_cell_counter: %llu observations need more than cell_count_max_mb = %lld", (unsigned long long)need, (long long)max_mb);
		return SVG_E_NOMEM;
	}
	void *nh = NULL, *nl = NULL;
	int rc = dmalloc(h, &nh, 8 * cap);
	if (!rc && (rc = dmalloc(h, &nl, 8 * cap))) { hipFree(nh); h->device_bytes -= 8 * cap; }
	if (rc) return rc;
	if (c->cnt[0] && (hipMemcpy(nh, c->d_hi, 8 * c->cnt[0], hipMemcpyDeviceToDevice) != hipSuccess ||
	                  hipMemcpy(nl, c->d_lo, 8 * c->cnt[0], hipMemcpyDeviceToDevice) != hipSuccess)) {
		hipFree(nh); hipFree(nl);
		h->device_bytes -= 16 * cap;
		svg_set_error("svg_cell_counter: device copy failed");
		return SVG_E_DEVICE;
	}
	hipFree(c->d_hi); hipFree(c->d_lo);
	h->device_bytes -= 16 * c->cap;
	c->d_hi = (uint64_t *)nh; c->d_lo = (uint64_t *)nl; c->cap = cap;
	return 0;
}

static int counter_quiesce(svg_cell_counter *c)
{
	svg_index *h = c->h;
	HIPCHK(hipSetDevice(h->device));
	if (h->last_pending) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_last, 0));
	HIPCHK(hipStreamSynchronize(h->stream));
	return 0;
}

extern "C" int svg_cell_counter_create(svg_index *h, int umi_length, int n_samples, svg_cell_counter **out)
{
	if (!h || !out) { svg_set_error("svg_cell_counter_create: NULL argument"); return SVG_E_ARG; }
	*out = NULL;
	if (umi_length < 1 || umi_length > SVG_CELL_MAX_UMI) {
		svg_set_error("svg_cell_counter_create: umi_length %d outside 1..%d", umi_length, SVG_CELL_MAX_UMI);
		return SVG_E_ARG;
	}
	if (n_samples < 1 || n_samples > SVG_CELL_MAX_SAMPLES) {
		svg_set_error("svg_cell_counter_create: n_samples %d outside 1..%d", n_samples, SVG_CELL_MAX_SAMPLES);
		return SVG_E_ARG;
	}
	svg_cell_counter *c = (svg_cell_counter *)calloc(1, sizeof *c);
	if (!c) { svg_set_error("out of host memory"); return SVG_E_NOMEM; }
	c->h = h; c->L = umi_length; c->n_samples = n_samples;
	c->cnt_bytes = 8 * (CNT_HEAD + 3 * ((size_t)n_samples + 1));
	c->cnt = (uint64_t *)calloc(1, c->cnt_bytes);
	if (!c->cnt) { free(c); svg_set_error("out of host memory"); return SVG_E_NOMEM; }
	void *d = NULL;
	int rc = hipSetDevice(h->device) == hipSuccess ? dmalloc(h, &d, c->cnt_bytes) : SVG_E_DEVICE;
	if (!rc && hipMemset(d, 0, c->cnt_bytes) != hipSuccess) { svg_set_error("svg_cell_counter_create: HIP error"); rc = SVG_E_DEVICE; }
	if (rc) { hipFree(d); free(c->cnt); free(c); return rc; }
	c->d_cnt = (unsigned long long *)d;
	*out = c;
	return 0;
}

extern "C" void svg_cell_counter_free(svg_cell_counter *c)
{
	if (!c) return;
	hipSetDevice(c->h->device);
	hipFree(c->d_hi); hipFree(c->d_lo); hipFree(c->d_cnt);
	c->h->device_bytes -= 16 * c->cap + c->cnt_bytes;
	free(c->cnt);
	free(c);
}

extern "C" int svg_cell_counter_reset(svg_cell_counter *c)
{
	if (!c) { svg_set_error("svg_cell_counter_reset: NULL argument"); return SVG_E_ARG; }
	int rc = counter_quiesce(c);
	if (rc) return rc;
	memset(c->cnt, 0, c->cnt_bytes);
	HIPCHK(hipMemset(c->d_cnt, 0, c->cnt_bytes));
	return 0;
}

extern "C" int svg_cell_counter_add(svg_cell_counter *c, const int32_t *sample, const int32_t *cell, const int64_t *gene,
                                    const char *umi_text, uint64_t n)
{
	if (!c || (n && (!sample || !cell || !gene || !umi_text))) { svg_set_error("svg_cell_counter_add: NULL argument"); return SVG_E_ARG; }
	if (!n) return 0;
	uint64_t *hi = (uint64_t *)malloc(16 * n), *lo = hi + n, m = 0, ds = 0, dc = 0;
	if (!hi) { svg_set_error("out of host memory"); return SVG_E_NOMEM; }
	int rc = 0;
	for (uint64_t i = 0; i < n && !rc; i++) {
		const uint64_t code = umi_encode(umi_text + i * (uint64_t)c->L, c->L);
		if (code == ~0ull) { svg_set_error("svg_cell_counter_add: observation %llu: a UMI character other than A/C/G/T/N", (unsigned long long)i); rc = SVG_E_ARG; }
		if (rc) break;
		if (sample[i] > c->n_samples) {
			svg_set_error("svg_cell_counter_add: observation %llu: sample %d of %d", (unsigned long long)i, sample[i], c->n_samples);
			rc = SVG_E_ARG;
		} else if (cell[i] >= SVG_CELL_MAX_CELLS) {
			svg_set_error("svg_cell_counter_add: observation %llu: cell %d does not fit 24 bits", (unsigned long long)i, cell[i]);
			rc = SVG_E_ARG;
		} else if (gene[i] < 0 || gene[i] > 0x7fffffffll) {
			svg_set_error("svg_cell_counter_add: observation %llu: gene %lld outside 0..2^31-1", (unsigned long long)i, (long long)gene[i]);
			rc = SVG_E_ARG;
		} else if (sample[i] <= 0) ds++;
		else if (cell[i] < 0) dc++;
		else {
			hi[m] = (uint64_t)sample[i] << 56 | (uint64_t)cell[i] << 32 | (uint64_t)gene[i];
			lo[m] = code;
			m++;
		}
	}
	if (!rc) rc = counter_quiesce(c);
	if (!rc) rc = counter_grow(c, c->cnt[0] + m);
	if (!rc && m && (hipMemcpy(c->d_hi + c->cnt[0], hi, 8 * m, hipMemcpyHostToDevice) != hipSuccess ||
	                 hipMemcpy(c->d_lo + c->cnt[0], lo, 8 * m, hipMemcpyHostToDevice) != hipSuccess)) {
		svg_set_error("svg_cell_counter_add: upload failed");
		rc = SVG_E_DEVICE;
	}
	free(hi);
	if (rc) return rc;
	c->cnt[0] += m; c->cnt[1] += ds; c->cnt[2] += dc;
	HIPCHK(hipMemcpy(c->d_cnt, c->cnt, c->cnt_bytes, hipMemcpyHostToDevice));
	return 0;
}

extern "C" int svg_cell_counter_tallies(svg_cell_counter *c, uint64_t *reads, uint64_t *mapped, uint64_t *assigned)
{
	if (!c || !reads || !mapped || !assigned) { svg_set_error("svg_cell_counter_tallies: NULL argument"); return SVG_E_ARG; }
	// (the host copy is the device's after every call that succeeded)
	const size_t k = (size_t)c->n_samples + 1;
	memcpy(reads, c->cnt + CNT_HEAD, 8 * k);
	memcpy(mapped, c->cnt + CNT_HEAD + k, 8 * k);
	memcpy(assigned, c->cnt + CNT_HEAD + 2 * k, 8 * k);
	return 0;
}

// ---- svg_cell_count_batch: the sink behind cell_align_run's chunks

struct CellCountSink;
static int count_run(svg_index *h, const svg_cell_align_params *p, const svg_packed_reads *reads, const svg_packed_reads *barcodes, CellCountSink *sp,
                     svg_cell_assigned *res);

struct CellCountSink {
	svg_cell_counter *c;
	const svg_packed_reads *umis;    // svg_cell_count_batch: the UMIs and sample numbers from the host
	const int32_t *sample_no;
	const svg_reads *names;          // svg_cell_count_names_batch: both, and the barcodes, from the parse kernel
	int mode, barcode_length;
	CellNamesRun *nr;
	void *d_ubases, *d_uxmask, *d_ustarts, *d_sample;
	size_t held;
	hipEvent_t ev[2];
};

static int sink_alloc(CellCountSink *s, void **p, size_t bytes)
{
	int rc = dmalloc(s->c->h, p, bytes);
	if (!rc) s->held += bytes;
	return rc;
}

const char *cell_count_who(CellCountSink *s) { return s->names ? "svg_cell_count_names_batch" : "svg_cell_count_batch"; }
bool cell_count_has_names(CellCountSink *s) { return s->names != NULL; }

static int sink_events(CellCountSink *s)
{
	if (s->c->h->timing)
		for (int i = 0; i < 2; i++)
			if (hipEventCreate(&s->ev[i]) != hipSuccess) { svg_set_error("%s: hipEventCreate failed", cell_count_who(s)); return SVG_E_DEVICE; }
	return 0;
}

int cell_count_begin(CellCountSink *s, uint64_t n, uint64_t chunk, hipStream_t st)
{
	svg_cell_counter *c = s->c;
	if (s->names) {
		int rc = cell_names_begin(c->h, cell_count_who(s), s->names, s->mode, s->barcode_length, c->L, n, chunk, st, &s->nr);
		return rc ? rc : sink_events(s);
	}
	const svg_packed_reads *u = s->umis;
	uint64_t nbases = 0;
	for (uint64_t i = 0; i < n; i++) {
		if (u->lens[i] != (uint16_t)c->L) {
			svg_set_error("svg_cell_count_batch: UMI %llu has %d bases (the counter's have %d)", (unsigned long long)i, (int)u->lens[i], c->L);
			return SVG_E_ARG;
		}
		if (!u->starts && (uint64_t)c->L > u->stride) {
			svg_set_error("svg_cell_count_batch: UMI %llu is longer than the stride", (unsigned long long)i);
			return SVG_E_ARG;
		}
		const uint64_t e = (u->starts ? u->starts[i] : i * u->stride) + (uint64_t)c->L;
		if (e > nbases) nbases = e;
	}
	const size_t bw = (size_t)((nbases + 15) / 16) * 4, xw = u->xmask ? (size_t)((nbases + 31) / 32) * 4 : 0;
	int rc;
	if ((rc = sink_alloc(s, &s->d_ubases, bw)) || (xw && (rc = sink_alloc(s, &s->d_uxmask, xw))) ||
	    (u->starts && (rc = sink_alloc(s, &s->d_ustarts, 8 * n))) || (rc = sink_alloc(s, &s->d_sample, 4 * n)))
		return rc;
	if (hipMemcpyAsync(s->d_ubases, u->bases, bw, hipMemcpyHostToDevice, st) != hipSuccess ||
	    (xw && hipMemcpyAsync(s->d_uxmask, u->xmask, xw, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    (u->starts && hipMemcpyAsync(s->d_ustarts, u->starts, 8 * n, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    hipMemcpyAsync(s->d_sample, s->sample_no, 4 * n, hipMemcpyHostToDevice, st) != hipSuccess) {
		svg_set_error("svg_cell_count_batch: upload failed");
		return SVG_E_DEVICE;
	}
	return sink_events(s);
}

// the parse kernel over the chunk's names, in front of the barcode kernel that reads its output
int cell_count_parse(CellCountSink *s, uint64_t first_read, uint64_t k, const uint32_t **d_bc_bases, const uint32_t **d_bc_xmask)
{
	if (!s->nr) return 0;
	int rc = cell_names_chunk(s->nr, first_read, k);
	if (rc) return rc;
	CellNamesView v;
	cell_names_view(s->nr, &v);
	*d_bc_bases = v.bc_bases;
	*d_bc_xmask = v.bc_xmask;
	return 0;
}

// the chunk's k reads from first_read on; its records start at rec_base, its gene lists (n_genes
// numbers) at gene_base.  The stream is idle when this is called (the assignment has synchronised)
int cell_count_chunk(CellCountSink *s, uint64_t first_read, uint64_t k, const svg_cell_aln_head *d_heads, uint64_t rec_base,
                     const svg_cell_hit *d_hits, const int32_t *d_genes, uint64_t gene_base, uint64_t n_genes, const int32_t *d_bc,
                     hipStream_t st)
{
	svg_cell_counter *c = s->c;
	unsigned long long n_now = 0;
	if (hipMemcpy(&n_now, c->d_cnt, 8, hipMemcpyDeviceToHost) != hipSuccess) { svg_set_error("%s: HIP error", cell_count_who(s)); return SVG_E_DEVICE; }
	const uint64_t keep = c->cnt[0];
	c->cnt[0] = n_now;               // (what counter_grow copies)
	int rc = counter_grow(c, n_now + n_genes);
	c->cnt[0] = keep;
	if (rc) return rc;
	ExpandParams ep;
	memset(&ep, 0, sizeof ep);
	ep.heads = d_heads; ep.hits = d_hits; ep.genes = d_genes; ep.bc = d_bc;
	if (s->nr) {
		CellNamesView v;
		cell_names_view(s->nr, &v);
		cell_names_time(s->nr);
		ep.sample = v.sample; ep.status = v.status;
		ep.ubases = v.umi_bases; ep.uxmask = v.umi_xmask;
		ep.ustride = SVG_CELL_NAME_STRIDE;
	} else {
		ep.sample = (const int32_t *)s->d_sample + first_read;
		ep.ubases = (const uint32_t *)s->d_ubases;
		ep.uxmask = (const uint32_t *)s->d_uxmask;
		ep.ustarts = s->d_ustarts ? (const uint64_t *)s->d_ustarts + first_read : NULL;
		ep.ustride = s->umis->stride;
		ep.ubase0 = first_read * s->umis->stride;
	}
	ep.rec_base = rec_base; ep.gene_base = gene_base; ep.cap = c->cap;
	ep.n = (uint32_t)k; ep.L = (uint32_t)c->L; ep.n_samples = c->n_samples;
	ep.hi = c->d_hi; ep.lo = c->d_lo; ep.cnt = c->d_cnt;
	if (s->ev[0]) hipEventRecord(s->ev[0], st);
	if (n_genes) hipLaunchKernelGGL(count_expand_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, ep);
	if (s->ev[0]) hipEventRecord(s->ev[1], st);
	hipLaunchKernelGGL(count_tally_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, ep);
	if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
		svg_set_error("%s: HIP error %s", cell_count_who(s), hipGetErrorString(hipGetLastError()));
		return SVG_E_DEVICE;
	}
	float ms = 0;
	if (s->ev[0] && hipEventElapsedTime(&ms, s->ev[0], s->ev[1]) == hipSuccess) c->h->cellcount_ms[0] += ms;
	return 0;
}

static void sink_free(CellCountSink *s)
{
	hipFree(s->d_ubases); hipFree(s->d_uxmask); hipFree(s->d_ustarts); hipFree(s->d_sample);
	cell_names_end(s->nr);
	for (int i = 0; i < 2; i++)
		if (s->ev[i]) hipEventDestroy(s->ev[i]);
	s->c->h->device_bytes -= s->held;
}

extern "C" int svg_cell_count_batch(svg_index *h, const svg_cell_align_params *p, const svg_packed_reads *reads,
                                    const svg_packed_reads *barcodes, const svg_packed_reads *umis, const int32_t *sample_no,
                                    svg_cell_counter *c, svg_cell_assigned *res)
{
	if (res) memset(res, 0, sizeof *res);
	if (!h || !p || !reads || !c || !umis || (reads->n_reads && !sample_no)) { svg_set_error("svg_cell_count_batch: NULL argument"); return SVG_E_ARG; }
	if (c->h != h) { svg_set_error("svg_cell_count_batch: the counter belongs to another handle"); return SVG_E_ARG; }
	if ((barcodes && barcodes->n_reads != reads->n_reads) || umis->n_reads != reads->n_reads) {
		svg_set_error("svg_cell_count_batch: %llu barcodes and %llu UMIs for %llu reads", (unsigned long long)(barcodes ? barcodes->n_reads : 0),
		              (unsigned long long)umis->n_reads, (unsigned long long)reads->n_reads);
		return SVG_E_ARG;
	}
	if (reads->n_reads && (!umis->bases || !umis->lens)) { svg_set_error("svg_cell_count_batch: NULL UMI buffer"); return SVG_E_ARG; }
	CellCountSink s;
	memset(&s, 0, sizeof s);
	s.c = c; s.umis = umis; s.sample_no = sample_no;
	return count_run(h, p, reads, barcodes, &s, res);
}

extern "C" int svg_cell_count_names_batch(svg_index *h, const svg_cell_align_params *p, const svg_packed_reads *reads, const svg_reads *names,
                                          int mode, svg_cell_counter *c, svg_cell_assigned *res)
{
	if (res) memset(res, 0, sizeof *res);
	if (!h || !p || !reads || !c || !names) { svg_set_error("svg_cell_count_names_batch: NULL argument"); return SVG_E_ARG; }
	if (c->h != h) { svg_set_error("svg_cell_count_names_batch: the counter belongs to another handle"); return SVG_E_ARG; }
	if (names->n_reads != reads->n_reads) {
		svg_set_error("svg_cell_count_names_batch: %llu names for %llu reads", (unsigned long long)names->n_reads, (unsigned long long)reads->n_reads);
		return SVG_E_ARG;
	}
	const int bl = cell_assign_barcode_length(h);
	if (!bl) { svg_set_error("svg_cell_count_names_batch: no whitelist (svg_cell_set_barcodes gives the barcode length)"); return SVG_E_ARG; }
	if (cell_names_samples(h) > c->n_samples) {
		svg_set_error("svg_cell_count_names_batch: a sample sheet of %d samples and a counter of %d", cell_names_samples(h), c->n_samples);
		return SVG_E_ARG;
	}
	CellCountSink s;
	memset(&s, 0, sizeof s);
	s.c = c; s.names = names; s.mode = mode; s.barcode_length = bl;
	return count_run(h, p, reads, NULL, &s, res);
}

// svg_cell_count_batch and svg_cell_count_names_batch behind their argument checks
static int count_run(svg_index *h, const svg_cell_align_params *p, const svg_packed_reads *reads, const svg_packed_reads *barcodes, CellCountSink *sp,
                     svg_cell_assigned *res)
{
	CellCountSink &s = *sp;
	svg_cell_counter *c = s.c;
	svg_cell_assigned tmp;
	memset(&tmp, 0, sizeof tmp);
	svg_cell_assigned *r = res ? res : &tmp;
	int rc = cell_align_run(h, p, reads, &r->alns, barcodes, &r->hits, &r->cell_barcode_no, &s, res == NULL);
	sink_free(&s);
	if (!rc && hipMemcpy(c->cnt, c->d_cnt, c->cnt_bytes, hipMemcpyDeviceToHost) != hipSuccess) { svg_set_error("%s: HIP error", cell_count_who(&s)); rc = SVG_E_DEVICE; }
	if (rc) {
		hipMemcpy(c->d_cnt, c->cnt, c->cnt_bytes, hipMemcpyHostToDevice);   // the counter as it was before the call
		svg_cell_assign_free(r);
		return rc;
	}
	if (!res) svg_cell_assign_free(&tmp);
	return 0;
}

// ---- svg_cell_counter_finish

struct Finish {
	svg_index *h;
	hipStream_t st;
	void *ptr[48];
	size_t bytes[48];
	int np;
	void *tmp;
	size_t tmp_bytes;
	hipEvent_t ev[6];
};

static int fin_alloc(Finish *f, void **p, size_t bytes)
{
	if (f->np == 48) { svg_set_error("svg_cell_counter_finish: buffer table full"); return SVG_E_DEVICE; }
	int rc = dmalloc(f->h, p, bytes);
	if (rc) return rc;
	f->ptr[f->np] = *p; f->bytes[f->np] = bytes; f->np++;
	return 0;
}

static void fin_free(Finish *f)
{
	for (int i = 0; i < f->np; i++) { hipFree(f->ptr[i]); f->h->device_bytes -= f->bytes[i]; }
	hipFree(f->tmp);
	f->h->device_bytes -= f->tmp_bytes;
	for (int i = 0; i < 6; i++)
		if (f->ev[i]) hipEventDestroy(f->ev[i]);
}

// a hipcub call in its two phases over the run's grow-only temporary buffer
template <class F> static int cub_run(Finish *f, F call)
{
	size_t need = 0;
	if (call((void *)NULL, need) != hipSuccess) { svg_set_error("svg_cell_counter_finish: hipcub sizing failed"); return SVG_E_DEVICE; }
	if (need > f->tmp_bytes) {
		hipStreamSynchronize(f->st);
		hipFree(f->tmp);
		f->h->device_bytes -= f->tmp_bytes;
		f->tmp = NULL; f->tmp_bytes = 0;
		int rc = dmalloc(f->h, &f->tmp, need);
		if (rc) return rc;
		f->tmp_bytes = need;
	}
	if (!need) need = 1;
	if (call(f->tmp, need) != hipSuccess) { svg_set_error("svg_cell_counter_finish: hipcub call failed: %s", hipGetErrorString(hipGetLastError())); return SVG_E_DEVICE; }
	return 0;
}

#define FA(p, type, count) do { void *_p = NULL; if ((rc = fin_alloc(&f, &_p, sizeof(type) * (size_t)(count)))) goto done; p = (type *)_p; } while (0)
#define FCUB(...) do { if ((rc = cub_run(&f, [&](void *t_, size_t &b_) { return __VA_ARGS__; }))) goto done; } while (0)
#define FSYNC() do { if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { \
	svg_set_error("svg_cell_counter_finish: HIP error %s", hipGetErrorString(hipGetLastError())); rc = SVG_E_DEVICE; goto done; } } while (0)
#define FMARK(k) do { if (f.ev[k]) hipEventRecord(f.ev[k], st); } while (0)
#define GRID(n) dim3((unsigned)(((n) + 255u) / 256u)), dim3(256), 0, st

extern "C" void svg_cell_counts_free(svg_cell_counts *out)
{
	if (!out) return;
	free(out->counts); free(out->count_first); free(out->removed_umis); free(out->entries); free(out->entry_first);
	memset(out, 0, sizeof *out);
}

extern "C" int svg_cell_counter_finish(svg_cell_counter *c, int want_entries, svg_cell_counts *out)
{
	if (!c || !out) { svg_set_error("svg_cell_counter_finish: NULL argument"); return SVG_E_ARG; }
	memset(out, 0, sizeof *out);
	if (c->cnt[4]) {
		svg_set_error("svg_cell_counter_finish: %llu read names refused (fewer than 3 fields, or a barcode or UMI past the name's end or with a character other than A/C/G/T/N; refused until svg_cell_counter_reset)",
		              (unsigned long long)c->cnt[4]);
		return SVG_E_ARG;
	}
	if (c->cnt[3]) {
		svg_set_error("svg_cell_counter_finish: %llu observations with a sample, cell or gene number outside its key field (refused until svg_cell_counter_reset)",
		              (unsigned long long)c->cnt[3]);
		return SVG_E_ARG;
	}
	svg_index *h = c->h;
	int rc = counter_quiesce(c);
	if (rc) return rc;
	hipStream_t st = h->stream;
	const int S = c->n_samples, L = c->L;
	const uint32_t n = (uint32_t)c->cnt[0];
	out->n_samples = (uint32_t)S; out->umi_length = (uint32_t)L;
	out->dropped_no_sample = c->cnt[1]; out->dropped_no_cell = c->cnt[2];
	out->count_first = (uint64_t *)calloc((size_t)S + 1, 8);
	out->entry_first = (uint64_t *)calloc((size_t)S + 1, 8);
	out->removed_umis = (uint64_t *)calloc((size_t)S, 8);
	if (!out->count_first || !out->entry_first || !out->removed_umis) { svg_cell_counts_free(out); svg_set_error("out of host memory"); return SVG_E_NOMEM; }
	if (!n) return 0;
	Finish f;
	memset(&f, 0, sizeof f);
	f.h = h; f.st = st;
	FinishParams fp;
	memset(&fp, 0, sizeof fp);
	uint64_t *t_hi, *t_lo, *s_hi, *s_lo, *key_b, *k64a, *k64b, *u_hi, *o_hi;
	uint32_t *idx2, *idx3, *key_a2, *sel, *sel2, *k32a, *k32b, *u_n, *o_n;
	uint32_t meta[5] = {0, 0, 0, 0, 0};
	uint32_t ne = 0, n2 = 0, nrows = 0;
	if (h->timing)
		for (int i = 0; i < 6; i++)
			if (hipEventCreate(&f.ev[i]) != hipSuccess) { svg_set_error("svg_cell_counter_finish: hipEventCreate failed"); rc = SVG_E_DEVICE; goto done; }
	fp.n = n;
	fp.mask_f = umi_half_mask(L, 0);
	fp.mask_s = umi_half_mask(L, 1);
	FA(fp.meta, uint32_t, 8);
	FA(fp.removed, unsigned long long, S);
	if (hipMemsetAsync(fp.meta, 0, 32, st) != hipSuccess || hipMemsetAsync(fp.removed, 0, 8 * (size_t)S, st) != hipSuccess) {
		svg_set_error("svg_cell_counter_finish: HIP error"); rc = SVG_E_DEVICE; goto done;
	}
	FMARK(0);
	// 1. the support count: the observations by (key, UMI), run-length into entries
	FA(t_hi, uint64_t, n); FA(t_lo, uint64_t, n); FA(s_hi, uint64_t, n); FA(s_lo, uint64_t, n);
	FCUB(hipcub::DeviceRadixSort::SortPairs(t_, b_, (const uint64_t *)c->d_lo, t_lo, (const uint64_t *)c->d_hi, t_hi, (int)n, 0, 3 * L, st));
	FCUB(hipcub::DeviceRadixSort::SortPairs(t_, b_, (const uint64_t *)t_hi, s_hi, (const uint64_t *)t_lo, s_lo, (int)n, 0, 64, st));
	fp.s_hi = s_hi; fp.s_lo = s_lo;
	FA(fp.flag, uint32_t, n); FA(fp.pos, uint32_t, n); FA(fp.e_start, uint32_t, (size_t)n + 1);
	hipLaunchKernelGGL(obs_head_kernel, GRID(n), fp);
	FCUB(hipcub::DeviceScan::ExclusiveSum(t_, b_, fp.flag, fp.pos, (int)n, st));
	hipLaunchKernelGGL(obs_start_kernel, GRID(n), fp);
	if (hipMemcpyAsync(meta, fp.meta, 4, hipMemcpyDeviceToHost, st) != hipSuccess) { svg_set_error("svg_cell_counter_finish: HIP error"); rc = SVG_E_DEVICE; goto done; }
	FSYNC();
	ne = meta[0];
	fp.ne = ne;
	FA(fp.e_hi0, uint64_t, ne); FA(fp.e_lo0, uint64_t, ne); FA(fp.supp0, uint32_t, ne); FA(fp.key_a, uint32_t, ne); FA(fp.idx, uint32_t, ne);
	hipLaunchKernelGGL(entry_kernel, GRID(ne), fp);
	// 2. step 1's order: stable by ~support, then by (sample, cell, gene); the UMI order is the entries' own
	FA(key_a2, uint32_t, ne); FA(idx2, uint32_t, ne); FA(idx3, uint32_t, ne); FA(key_b, uint64_t, ne);
	FA(fp.e_hi, uint64_t, ne); FA(fp.e_lo, uint64_t, ne); FA(fp.supp, uint32_t, ne); FA(fp.supp_after, uint32_t, ne);
	FA(fp.acceptor, uint32_t, ne); FA(fp.outcome, uint32_t, ne); FA(fp.counted, uint32_t, ne);
	FA(fp.sec_start, uint32_t, (size_t)ne + 1); FA(fp.big, uint32_t, ne / (U_SMALL + 1) + 1);
	FA(fp.spill_code, uint64_t, ne); FA(fp.spill_idx, uint32_t, ne);
	FCUB(hipcub::DeviceRadixSort::SortPairs(t_, b_, (const uint32_t *)fp.key_a, key_a2, (const uint32_t *)fp.idx, idx2, (int)ne, 0, 32, st));
	hipLaunchKernelGGL(gather_hi_kernel, GRID(ne), (const uint64_t *)fp.e_hi0, (const uint32_t *)idx2, key_b, ne);
	FCUB(hipcub::DeviceRadixSort::SortPairs(t_, b_, (const uint64_t *)key_b, fp.e_hi, (const uint32_t *)idx2, idx3, (int)ne, 0, 64, st));
	hipLaunchKernelGGL(order1_kernel, GRID(ne), fp, (const uint32_t *)idx3);
	FCUB(hipcub::DeviceScan::ExclusiveSum(t_, b_, fp.flag, fp.pos, (int)ne, st));
	hipLaunchKernelGGL(section_kernel, GRID(ne), fp);
	FMARK(1);
	// 3. step 1
	hipLaunchKernelGGL(step1_lane_kernel, GRID(ne), fp);
	FMARK(2);
	hipLaunchKernelGGL(step1_wave_kernel, dim3((unsigned)(h->n_cu > 0 ? h->n_cu * 4 : 256)), dim3(64), 0, st, fp);
	FMARK(3);
	// 4. step 2: the survivors by (sample, cell, UMI, support descending, gene)
	hipLaunchKernelGGL(survivor_kernel, GRID(ne), fp);
	FA(sel, uint32_t, ne); FA(sel2, uint32_t, ne);
	FCUB(hipcub::DeviceSelect::Flagged(t_, b_, hipcub::CountingInputIterator<uint32_t>(0u), fp.flag, sel, fp.meta + 3, (int)ne, st));
	if (hipMemcpyAsync(meta, fp.meta, 20, hipMemcpyDeviceToHost, st) != hipSuccess) { svg_set_error("svg_cell_counter_finish: HIP error"); rc = SVG_E_DEVICE; goto done; }
	FSYNC();
	n2 = meta[3];
	fp.n2 = n2;
	if (n2) {
		FA(k64a, uint64_t, n2); FA(k64b, uint64_t, n2); FA(k32a, uint32_t, n2); FA(k32b, uint32_t, n2);
		hipLaunchKernelGGL(key2_kernel, GRID(n2), fp, (const uint32_t *)sel, k64a, k32a, 0);
		FCUB(hipcub::DeviceRadixSort::SortPairs(t_, b_, (const uint64_t *)k64a, k64b, (const uint32_t *)sel, sel2, (int)n2, 0, 64, st));
		hipLaunchKernelGGL(key2_kernel, GRID(n2), fp, (const uint32_t *)sel2, k64a, k32a, 1);
		FCUB(hipcub::DeviceRadixSort::SortPairs(t_, b_, (const uint64_t *)k64a, k64b, (const uint32_t *)sel2, sel, (int)n2, 0, 3 * L, st));
		hipLaunchKernelGGL(key2_kernel, GRID(n2), fp, (const uint32_t *)sel, k64a, k32a, 2);
		FCUB(hipcub::DeviceRadixSort::SortPairs(t_, b_, (const uint32_t *)k32a, k32b, (const uint32_t *)sel, sel2, (int)n2, 0, 32, st));
		fp.order = sel2;
		hipLaunchKernelGGL(step2_kernel, GRID(n2), fp);
	}
	FMARK(4);
	// 5. the count table: the counted entries of every (sample, cell, gene), the rows above zero
	FA(u_hi, uint64_t, ne); FA(u_n, uint32_t, ne); FA(o_hi, uint64_t, ne); FA(o_n, uint32_t, ne);
	FCUB(hipcub::DeviceReduce::ReduceByKey(t_, b_, (const uint64_t *)fp.e_hi, u_hi, (const uint32_t *)fp.counted, u_n, fp.meta + 5, hipcub::Sum(), (int)ne, st));
	if (hipMemcpyAsync(meta, fp.meta + 5, 4, hipMemcpyDeviceToHost, st) != hipSuccess) { svg_set_error("svg_cell_counter_finish: HIP error"); rc = SVG_E_DEVICE; goto done; }
	FSYNC();
	{
		const uint32_t runs = meta[0];
		FCUB(hipcub::DeviceSelect::Flagged(t_, b_, (const uint64_t *)u_hi, (const uint32_t *)u_n, o_hi, fp.meta + 4, (int)runs, st));
		FCUB(hipcub::DeviceSelect::Flagged(t_, b_, (const uint32_t *)u_n, (const uint32_t *)u_n, o_n, fp.meta + 4, (int)runs, st));
	}
	FMARK(5);
	if (hipMemcpyAsync(meta, fp.meta + 4, 4, hipMemcpyDeviceToHost, st) != hipSuccess) { svg_set_error("svg_cell_counter_finish: HIP error"); rc = SVG_E_DEVICE; goto done; }
	FSYNC();
	nrows = meta[0];
	if (f.ev[0])
		for (int i = 0; i < 5; i++) {
			float ms = 0;
			if (hipEventElapsedTime(&ms, f.ev[i], f.ev[i + 1]) == hipSuccess) h->cellcount_ms[i + 1] += ms;
		}
	{
		uint64_t *hk = (uint64_t *)malloc(8 * ((size_t)nrows + 1));
		uint32_t *hn = (uint32_t *)malloc(4 * ((size_t)nrows + 1));
		out->counts = (svg_cell_count *)malloc(sizeof(svg_cell_count) * ((size_t)nrows + 1));
		unsigned long long *rem = (unsigned long long *)malloc(8 * (size_t)S);
		if (!hk || !hn || !out->counts || !rem) { free(hk); free(hn); free(rem); svg_set_error("out of host memory"); rc = SVG_E_NOMEM; goto done; }
		if ((nrows && (hipMemcpy(hk, o_hi, 8 * (size_t)nrows, hipMemcpyDeviceToHost) != hipSuccess ||
		               hipMemcpy(hn, o_n, 4 * (size_t)nrows, hipMemcpyDeviceToHost) != hipSuccess)) ||
		    hipMemcpy(rem, fp.removed, 8 * (size_t)S, hipMemcpyDeviceToHost) != hipSuccess) {
			free(hk); free(hn); free(rem);
			svg_set_error("svg_cell_counter_finish: download failed"); rc = SVG_E_DEVICE; goto done;
		}
		for (uint32_t i = 0; i < nrows; i++) {
			svg_cell_count *q = out->counts + i;
			q->sample = (int32_t)(hk[i] >> 56); q->cell = (int32_t)((hk[i] >> 32) & 0xffffffu); q->gene = (int32_t)(uint32_t)hk[i];
			q->n_umis = hn[i];
			out->count_first[q->sample]++;
		}
		for (int s = 0; s < S; s++) { out->count_first[s + 1] += out->count_first[s]; out->removed_umis[s] = rem[s]; }
		out->n_counts = nrows;
		free(hk); free(hn); free(rem);
	}
	if (want_entries) {
		uint64_t *hh = (uint64_t *)malloc(8 * (size_t)ne), *hl = (uint64_t *)malloc(8 * (size_t)ne);
		uint32_t *hs = (uint32_t *)malloc(16 * (size_t)ne);
		out->entries = (svg_cell_umi_entry *)calloc(ne, sizeof(svg_cell_umi_entry));
		if (!hh || !hl || !hs || !out->entries) { free(hh); free(hl); free(hs); svg_set_error("out of host memory"); rc = SVG_E_NOMEM; goto done; }
		uint32_t *ha = hs + ne, *hacc = hs + 2 * (size_t)ne, *ho = hs + 3 * (size_t)ne;
		if (hipMemcpy(hh, fp.e_hi, 8 * (size_t)ne, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hl, fp.e_lo, 8 * (size_t)ne, hipMemcpyDeviceToHost) != hipSuccess ||
		    hipMemcpy(hs, fp.supp, 4 * (size_t)ne, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(ha, fp.supp_after, 4 * (size_t)ne, hipMemcpyDeviceToHost) != hipSuccess ||
		    hipMemcpy(hacc, fp.acceptor, 4 * (size_t)ne, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(ho, fp.outcome, 4 * (size_t)ne, hipMemcpyDeviceToHost) != hipSuccess) {
			free(hh); free(hl); free(hs);
			svg_set_error("svg_cell_counter_finish: download failed"); rc = SVG_E_DEVICE; goto done;
		}
		for (uint32_t i = 0; i < ne; i++) {
			svg_cell_umi_entry *q = out->entries + i;
			q->sample = (int32_t)(hh[i] >> 56); q->cell = (int32_t)((hh[i] >> 32) & 0xffffffu); q->gene = (int32_t)(uint32_t)hh[i];
			q->support = hs[i]; q->support_merged = ha[i]; q->outcome = ho[i];
			umi_decode(hl[i], L, q->umi);
			if (hacc[i] != U_NONE && hacc[i] < ne) umi_decode(hl[hacc[i]], L, q->acceptor_umi);
			out->entry_first[q->sample]++;
		}
		for (int s = 0; s < S; s++) out->entry_first[s + 1] += out->entry_first[s];
		out->n_entries = ne;
		free(hh); free(hl); free(hs);
	}
done:
	if (rc) hipStreamSynchronize(st);
	fin_free(&f);
	if (rc) svg_cell_counts_free(out);
	return rc;
}

static_assert(sizeof(svg_cell_count) == 16 && sizeof(svg_cell_umi_entry) == 52, "svg_cell_count / svg_cell_umi_entry layout");

extern "C" int svg_cell_count_timing(svg_index *h, double ms[6])
{
	if (!h || !ms) { svg_set_error("svg_cell_count_timing: NULL argument"); return SVG_E_ARG; }
	for (int i = 0; i < 6; i++) { ms[i] = h->cellcount_ms[i]; h->cellcount_ms[i] = 0; }
	return 0;
}
