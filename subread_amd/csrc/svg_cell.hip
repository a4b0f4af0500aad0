// svg_cell.hip -- cellCounts' voting step for a batch of reads (include/subread_vote.h
// svg_cell_vote_batch): cellCounts_do_voting's lookups (cell-counts.c:3079-3101) and
// cellCounts_process_copy_ptrs_to_votes (cell-counts.c:2786-2881) on the GPU.
//
// Three steps per chunk of reads:
//   cell_probe_kernel  thread = (read, strand, subread): the subread's 16-mer key from the 2-bit
//       packed read, then the key's equal-key run (svg_keylookup.h, svg_probe_keys's lookup) as
//       (global index of the run's first item, run length), 8 bytes per probe, slot-major
//       ([strand * 20 + subread][read]) so that neighbouring lanes of the tally read neighbours.
//   cell_tally_kernel  lane = read: the reference's sort of the 2 * applied subread numbers by
//       run length (quick_sort_run's Lomuto partitions, core.c:4694-4714, on an explicit stack:
//       the partitions of disjoint ranges do not depend on the order they are made in, so the
//       larger side is stacked and the stack holds at most 5 ranges), then the tally into the 17 x 3
//       table.  Per lane in LDS: position and votes | toli | strand of the 51 slots, the run
//       lengths, the permutation, the stack.  The indel recorder and the coverage go straight
//       into the read's 51 staging records in HBM, which have the output's format.
//   cell_scan_kernel, cell_compact_kernel  exclusive sum of the reads' slot counts (one block),
//       then the used staging records copied to their place in the compacted array.
// The wave of the tally runs as long as its heaviest lane.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "subread_vote.h"
#include "svg_internal.h"
#include "svg_device.h"
#include "svg_keylookup.h"
#include "svg_cell.h"

// cellCounts' subread plan (cell-counts.c:3079-3082, C's truncating divisions): the step in
// 1/65536 bases and the subreads per strand.  Lengths 16 .. 15 + gap have a span <= 0: the step
// is clamped up to the gap and one subread at offset 0 is left.
__device__ __forceinline__ int cell_plan(int len, int gap, int total, int &step)
{
	const int span = (int)((uint32_t)(len - 15 - gap) << 16);
	step = span / (total - 1);
	if (step < (gap << 16)) step = gap << 16;
	return 1 + span / step;
}

// the key (genekey2int) of the 16 bases at offset off of strand s of a read of len bases at
// `base`.  Strand 0 is the packed window itself.  Strand 1 is the window at len - 16 - off
// complemented (~code) and reversed; reverse_read leaves an exception base 'N' (code 3).
__device__ __forceinline__ uint32_t cell_key(const CellParams &cp, uint64_t base, int len, int s, int off)
{
	const uint64_t k0 = base + (uint64_t)(s ? len - 16 - off : off);
	const uint32_t *bw = cp.bases + (k0 >> 4);
	const uint32_t s2 = 2u * (uint32_t)(k0 & 15u);
	const uint32_t W = s2 ? (bw[0] << s2) | (bw[1] >> (32u - s2)) : bw[0];
	if (!s) return W;
	uint32_t X2 = 0;
	if (cp.xmask) {
		const uint32_t *xw = cp.xmask + (k0 >> 5);
		const uint32_t s1 = (uint32_t)(k0 & 31u);
		// bases k0..k0+15 (the next word only when they reach into it)
		uint32_t t = (s1 > 16u ? (xw[0] << s1) | (xw[1] >> (32u - s1)) : xw[0] << s1) >> 16;
		t = (t | (t << 8)) & 0x00ff00ffu;
		t = (t | (t << 4)) & 0x0f0f0f0fu;
		t = (t | (t << 2)) & 0x33333333u;
		t = (t | (t << 1)) & 0x55555555u;
		X2 = t | (t << 1);   // base i -> bits 31-2i .. 30-2i
	}
	const uint32_t v = __builtin_bitreverse32(~W | X2);
	return ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
}

template <int IMG>
__global__ void __launch_bounds__(256) cell_probe_kernel(CellParams cp)
{
	const uint64_t total = (uint64_t)cp.n * (2 * C_SUB);
	for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256u) {
		const uint32_t slot = (uint32_t)(t / cp.n), r = (uint32_t)(t - (uint64_t)slot * cp.n);
		const int s = slot >= C_SUB ? 1 : 0, k = (int)slot - C_SUB * s;
		const int len = cp.lens[r];
		if (len < 16) continue;
		int step;
		if (k >= cell_plan(len, cp.gap, cp.total_subreads, step)) continue;
		const uint32_t key = cell_key(cp, cell_read_base(cp, r), len, s, (step * k) >> 16);
		uint32_t f, c;
		const uint32_t b = key_run<IMG>(cp.kt, key, f, c);
		cp.probes[(size_t)slot * cp.n + r] = make_uint2(c ? cp.kt.bstart[b] + f : 0u, c);
	}
}

__global__ void __launch_bounds__(64) cell_tally_kernel(CellParams cp)
{
	__shared__ uint32_t s_pos[C_SLOTS][64];
	__shared__ uint32_t s_meta[C_SLOTS][64];    // votes | toli << 16 | strand << 24
	__shared__ uint32_t s_cnt[2 * C_SUB][64];
	__shared__ uint8_t s_ord[2 * C_SUB][64];
	__shared__ uint16_t s_stk[C_STACK][64];
	const int L = (int)threadIdx.x;
	const uint32_t r = blockIdx.x * 64u + threadIdx.x;
	if (r >= cp.n) return;
	const int len = cp.lens[r];
	int step = 0, applied = 0, max_vote = 0, n_slots = 0;
	uint64_t items = 0;                         // 2 bits per row
	svg_cell_slot *const stage = cp.staging + (size_t)r * C_SLOTS;
	if (len >= 16) {                            // cell-counts.c:3077
		applied = cell_plan(len, cp.gap, cp.total_subreads, step);
		const int subreads = 2 * applied;
		for (int i = 0; i < subreads; i++) {
			const int s = i >= applied ? 1 : 0;
			s_cnt[i][L] = cp.probes[(size_t)(s * C_SUB + i - s * applied) * cp.n + r].y;
			s_ord[i][L] = (uint8_t)i;
		}
		// quick_sort_run (core.c:4694-4714): pivot last, compare <= 0, ties keep the exchanges
		{
			int lo = 0, hi = subreads - 1, sp = 0;
			for (;;) {
				const uint32_t pv = s_cnt[s_ord[hi][L]][L];
				int i = lo - 1;
				for (int j = lo; j < hi; j++) {
					const uint8_t oj = s_ord[j][L];
					if (s_cnt[oj][L] <= pv) {
						i++;
						s_ord[j][L] = s_ord[i][L];
						s_ord[i][L] = oj;
					}
				}
				{
					const uint8_t t = s_ord[i + 1][L];
					s_ord[i + 1][L] = s_ord[hi][L];
					s_ord[hi][L] = t;
				}
				const bool left = i > lo, right = hi > i + 2;
				if (left && right) {
					// the larger side waits; the side gone on with at least halves each time, so
					// 40 -> 19 -> 9 -> 4 -> 1: at most 5 ranges wait
					if (i - lo + 1 >= hi - i - 1) { s_stk[sp++][L] = (uint16_t)(lo | (i << 8)); lo = i + 2; }
					else { s_stk[sp++][L] = (uint16_t)((i + 2) | (hi << 8)); hi = i; }
				} else if (left) hi = i;
				else if (right) lo = i + 2;
				else {
					if (!sp) break;
					const uint16_t e = s_stk[--sp][L];
					lo = e & 255;
					hi = e >> 8;
				}
			}
		}
		const uint32_t seed = s_cnt[s_ord[subreads - 1][L]][L];
		const int I = cp.max_indel;
		for (int x1 = 0; x1 < subreads; x1++) {
			const int myno = s_ord[x1][L];
			const uint32_t has = s_cnt[myno][L];
			if (!has) continue;
			const int s = myno >= applied ? 1 : 0, k = myno - s * applied;
			const int16_t p1 = (int16_t)(k + 1), offset = (int16_t)((step * k) >> 16), of16 = (int16_t)(offset + 16);
			const uint32_t *run = cp.vals + cp.probes[(size_t)(s * C_SUB + k) * cp.n + r].x;
			// (the reference's sum is an int: the same residues while seed + 66889 * has < 2^31,
			// i.e. for hit lists of up to 32,000 items -- the limit subread_vote.h states)
			uint32_t sum = seed;
			for (uint32_t x2 = 0; x2 < has; x2++) {
				const uint32_t kv = run[sum % has] - (uint32_t)offset;
				sum += C_PRIME;
				const int home = (int)((kv / 5u) % SVG_CELL_ROWS);
				const int homelen = (int)((items >> (2 * home)) & 3u);
				bool found = false;
				for (int q = 0; q < 3 && !found; q++) {          // iix = 0, +5, -5
					const int row = q == 0 ? home : (int)(((q == 1 ? kv + 5u : kv - 5u) / 5u) % SVG_CELL_ROWS);
					const int n = (int)((items >> (2 * row)) & 3u);
					for (int it = 0; it < n; it++) {
						const int idx = row * SVG_CELL_SPACE + it;
						const int dist = (int)(kv - s_pos[idx][L]);
						const uint32_t meta = s_meta[idx][L];
						if (dist < -I || dist > I || (int)(meta >> 24) != s) continue;
						svg_cell_slot *sl = stage + idx;
						int toli = (int)((meta >> 16) & 255u);
						bool known = false;
						for (int t = 0; t < toli; t += 3)
							if (sl->indel_recorder[t + 2] == dist) {
								if (sl->indel_recorder[t] > p1) sl->indel_recorder[t] = p1;
								if (sl->indel_recorder[t + 1] < p1) sl->indel_recorder[t + 1] = p1;
								known = true;
								break;
							}
						if (toli < SVG_CELL_RECORDER && !known) {
							sl->indel_recorder[toli] = p1;
							sl->indel_recorder[toli + 1] = p1;
							sl->indel_recorder[toli + 2] = (int16_t)dist;
							toli += 3;
						}
						const int votes = (int)(meta & 0xffffu) + 1;
						if (max_vote < votes) max_vote = votes;
						if (offset < sl->coverage_start) sl->coverage_start = offset;
						if (of16 > sl->coverage_end) sl->coverage_end = of16;
						s_meta[idx][L] = (uint32_t)votes | ((uint32_t)toli << 16) | ((uint32_t)s << 24);
						found = true;
						break;
					}
				}
				if (!found && homelen < SVG_CELL_SPACE) {
					const int idx = home * SVG_CELL_SPACE + homelen;
					svg_cell_slot *sl = stage + idx;
					items += 1ull << (2 * home);
					s_pos[idx][L] = kv;
					s_meta[idx][L] = 1u | (3u << 16) | ((uint32_t)s << 24);
					sl->indel_recorder[0] = p1;
					sl->indel_recorder[1] = p1;
					sl->indel_recorder[2] = 0;
					sl->coverage_start = offset;
					sl->coverage_end = of16;
					if (max_vote == 0) max_vote = 1;
				}
			}
		}
		// the LDS half of the used slots into their staging records; recorder zero from toli on
		for (int row = 0; row < SVG_CELL_ROWS; row++) {
			const int n = (int)((items >> (2 * row)) & 3u);
			n_slots += n;
			for (int it = 0; it < n; it++) {
				const int idx = row * SVG_CELL_SPACE + it;
				const uint32_t meta = s_meta[idx][L];
				svg_cell_slot *sl = stage + idx;
				sl->pos = s_pos[idx][L];
				sl->mask = (meta >> 24) ? C_NEG : 0;
				sl->votes = (int16_t)(meta & 0xffffu);
				sl->toli = (uint8_t)((meta >> 16) & 255u);
				sl->_pad = 0;
				for (int t = (int)((meta >> 16) & 255u); t < SVG_CELL_RECORDER; t++) sl->indel_recorder[t] = 0;
			}
		}
	}
	// the head (first_slot: cell_scan_kernel)
	uint32_t w[6];
	w[0] = (uint32_t)n_slots | ((uint32_t)(uint16_t)max_vote << 16);
	w[1] = (uint32_t)applied | ((uint32_t)(items & 3u) << 16) | ((uint32_t)((items >> 2) & 3u) << 24);
#pragma unroll
	for (int q = 0; q < 4; q++) {
		uint32_t v = 0;
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int row = 2 + 4 * q + j;
			if (row < SVG_CELL_ROWS) v |= (uint32_t)((items >> (2 * row)) & 3u) << (8 * j);
		}
		w[2 + q] = v;
	}
	uint32_t *hw = (uint32_t *)(cp.heads + r);
	hw[0] = 0; hw[1] = 0;
#pragma unroll
	for (int q = 0; q < 6; q++) hw[2 + q] = w[q];
}

// heads[r].first_slot = slot_base + (slots of the chunk's reads before r) for every voted read; *total = the chunk's slots
__global__ void __launch_bounds__(1024) cell_scan_kernel(CellParams cp)
{
	__shared__ uint32_t part[1024];
	const uint32_t tid = threadIdx.x, per = (cp.n + 1023u) / 1024u;
	const uint32_t lo = min(cp.n, tid * per), hi = min(cp.n, lo + per);
	uint32_t sum = 0;
	for (uint32_t r = lo; r < hi; r++) sum += cp.heads[r].n_slots;
	part[tid] = sum;
	__syncthreads();
	for (uint32_t d = 1; d < 1024u; d <<= 1) {
		const uint32_t v = tid >= d ? part[tid - d] : 0u;
		__syncthreads();
		part[tid] += v;
		__syncthreads();
	}
	uint64_t at = cp.slot_base + (part[tid] - sum);
	for (uint32_t r = lo; r < hi; r++) {
		if (cp.heads[r].applied_subreads) cp.heads[r].first_slot = at;   // (a skipped read keeps its zero head)
		at += cp.heads[r].n_slots;
	}
	if (tid == 1023u) *cp.total = part[1023];
}

// thread = (read, table slot): a used slot's staging record to its place in the compacted array
__global__ void __launch_bounds__(256) cell_compact_kernel(CellParams cp)
{
	const uint64_t total = (uint64_t)cp.n * C_SLOTS;
	for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256u) {
		const uint32_t r = (uint32_t)(t / C_SLOTS), idx = (uint32_t)(t - (uint64_t)r * C_SLOTS);
		const uint32_t row = idx / SVG_CELL_SPACE, it = idx - row * SVG_CELL_SPACE;
		const svg_cell_head *h = cp.heads + r;
		if (it >= h->items[row]) continue;
		uint64_t at = h->first_slot - cp.slot_base + it;
		for (uint32_t q = 0; q < row; q++) at += h->items[q];
		const uint2 *src = (const uint2 *)(cp.staging + t);
		uint2 *dst = (uint2 *)(cp.compact + at);
#pragma unroll
		for (int q = 0; q < (int)(sizeof(svg_cell_slot) / 8); q++) dst[q] = src[q];
	}
}

void cell_launch_vote(const CellParams &cp, int img, int n_cu, hipStream_t st, hipEvent_t mid)
{
	const uint64_t k = cp.n, bmax = (uint64_t)n_cu * 16;
	uint64_t pblocks = (k * 2 * C_SUB + 255) / 256;
	if (pblocks > bmax) pblocks = bmax;
	if (img == KEYS_CODE) hipLaunchKernelGGL(cell_probe_kernel<KEYS_CODE>, dim3((unsigned)pblocks), dim3(256), 0, st, cp);
	else if (img == KEYS_KHASH) hipLaunchKernelGGL(cell_probe_kernel<KEYS_KHASH>, dim3((unsigned)pblocks), dim3(256), 0, st, cp);
	else hipLaunchKernelGGL(cell_probe_kernel<KEYS_LITERAL>, dim3((unsigned)pblocks), dim3(256), 0, st, cp);
	if (mid) hipEventRecord(mid, st);
	hipLaunchKernelGGL(cell_tally_kernel, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, st, cp);
}

extern "C" void svg_cell_vote_free(svg_cell_votes *res)
{
	if (!res) return;
	free(res->heads);
	free(res->slots);
	memset(res, 0, sizeof *res);
}

static_assert(sizeof(svg_cell_head) == 32 && sizeof(svg_cell_slot) == 56, "svg_cell record layout");

extern "C" int svg_cell_vote_batch(svg_index *h, const svg_cell_params *p, const svg_packed_reads *reads, svg_cell_votes *res)
{
	if (!h || !p || !reads || !res) { svg_set_error("svg_cell_vote_batch: NULL argument"); return SVG_E_ARG; }
	memset(res, 0, sizeof *res);
	if (h->nblocks > 1) {
		svg_set_error("svg_cell_vote_batch: an index of %d blocks (cellCounts takes a one-block index)", h->nblocks);
		return SVG_E_UNSUPPORTED;
	}
	if (p->total_subreads < 7 || p->total_subreads > C_SUB) {
		svg_set_error("svg_cell_vote_batch: total_subreads %d outside 7..%d", p->total_subreads, C_SUB);
		return SVG_E_ARG;
	}
	if (p->max_indel_length != 5) {
		svg_set_error("svg_cell_vote_batch: max_indel_length %d (cellCounts votes with 5)", p->max_indel_length);
		return SVG_E_ARG;
	}
	const uint64_t n = reads->n_reads;
	if (n == 0) return 0;
	if (!reads->bases || !reads->lens) { svg_set_error("svg_cell_vote_batch: NULL read buffer"); return SVG_E_ARG; }
	uint64_t nbases = 0;
	for (uint64_t r = 0; r < n; r++) {
		if (reads->lens[r] > SVG_CELL_MAX_READ_LENGTH) {
			svg_set_error("svg_cell_vote_batch: read %llu has %d bases (at most %d)", (unsigned long long)r, (int)reads->lens[r],
			              SVG_CELL_MAX_READ_LENGTH);
			return SVG_E_ARG;
		}
		if (!reads->starts && reads->lens[r] > reads->stride) {
			svg_set_error("svg_cell_vote_batch: read %llu is longer than the stride", (unsigned long long)r);
			return SVG_E_ARG;
		}
		const uint64_t e = (reads->starts ? reads->starts[r] : r * reads->stride) + reads->lens[r];
		if (e > nbases) nbases = e;
	}
	HIPCHK(hipSetDevice(h->device));
	hipStream_t st = h->stream;
	if (h->last_pending) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));
	const uint64_t CH = 1u << 17;   // reads per chunk: 51 staging + 51 compacted records each
	const uint64_t m = n < CH ? n : CH;
	const size_t bw = (size_t)((nbases + 15) / 16) * 4, xw = reads->xmask ? (size_t)((nbases + 31) / 32) * 4 : 0;
	const size_t sizes[8] = {bw + 8, xw + 8, reads->starts ? 8 * n : 0, 2 * n, sizeof(uint2) * 2 * C_SUB * m,
	                         sizeof(svg_cell_head) * m, sizeof(svg_cell_slot) * C_SLOTS * m, sizeof(svg_cell_slot) * C_SLOTS * m};
	void *d[9] = {NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL};
	uint64_t held = 0, nslots = 0, cap = 0;
	int rc = 0;
	for (int i = 0; i < 9 && !rc; i++) {
		const size_t sz = i < 8 ? sizes[i] : 8;
		if (!sz) continue;
		if (!(rc = dmalloc(h, &d[i], sz))) held += sz;
	}
	res->heads = (svg_cell_head *)malloc(sizeof(svg_cell_head) * n);
	if (!rc && !res->heads) { svg_set_error("out of host memory"); rc = SVG_E_NOMEM; }
	if (!rc && (hipMemcpyAsync(d[0], reads->bases, bw, hipMemcpyHostToDevice, st) != hipSuccess ||
	            (xw && hipMemcpyAsync(d[1], reads->xmask, xw, hipMemcpyHostToDevice, st) != hipSuccess) ||
	            (reads->starts && hipMemcpyAsync(d[2], reads->starts, 8 * n, hipMemcpyHostToDevice, st) != hipSuccess) ||
	            hipMemcpyAsync(d[3], reads->lens, 2 * n, hipMemcpyHostToDevice, st) != hipSuccess)) {
		svg_set_error("svg_cell_vote_batch: upload failed");
		rc = SVG_E_DEVICE;
	}
	const int img = key_image(h);
	for (uint64_t o = 0; o < n && !rc; o += m) {
		const uint64_t k = n - o < m ? n - o : m;
		CellParams cp;
		memset(&cp, 0, sizeof cp);
		cp.kt = key_table(h);
		cp.vals = h->dix.vals;
		cp.gap = h->dix.gap;
		cp.total_subreads = p->total_subreads;
		cp.max_indel = p->max_indel_length;
		cp.bases = (const uint32_t *)d[0];
		cp.xmask = xw ? (const uint32_t *)d[1] : NULL;
		cp.starts = reads->starts ? (const uint64_t *)d[2] + o : NULL;
		cp.stride = reads->stride;
		cp.base0 = o * reads->stride;
		cp.lens = (const uint16_t *)d[3] + o;
		cp.n = (uint32_t)k;
		cp.probes = (uint2 *)d[4];
		cp.heads = (svg_cell_head *)d[5];
		cp.staging = (svg_cell_slot *)d[6];
		cp.compact = (svg_cell_slot *)d[7];
		cp.slot_base = nslots;
		cp.total = (uint64_t *)d[8];
		uint64_t cblocks = (k * C_SLOTS + 255) / 256;
		const uint64_t bmax = (uint64_t)h->n_cu * 16;
		if (cblocks > bmax) cblocks = bmax;
		cell_launch_vote(cp, img, h->n_cu, st);
		hipLaunchKernelGGL(cell_scan_kernel, dim3(1), dim3(1024), 0, st, cp);
		hipLaunchKernelGGL(cell_compact_kernel, dim3((unsigned)cblocks), dim3(256), 0, st, cp);
		uint64_t used = 0;
		if (hipGetLastError() != hipSuccess ||
		    hipMemcpyAsync(res->heads + o, d[5], sizeof(svg_cell_head) * k, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipMemcpyAsync(&used, d[8], 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
			svg_set_error("svg_cell_vote_batch: HIP error %s", hipGetErrorString(hipGetLastError()));
			rc = SVG_E_DEVICE;
			break;
		}
		if (nslots + used > cap) {
			// room for the remaining reads at this chunk's rate, so that few chunks grow it
			cap = nslots + used + used * ((n - o - k + k - 1) / k);
			svg_cell_slot *g = (svg_cell_slot *)realloc(res->slots, sizeof(svg_cell_slot) * cap);
			if (!g) { svg_set_error("out of host memory"); rc = SVG_E_NOMEM; break; }
			res->slots = g;
		}
		if (used && hipMemcpy(res->slots + nslots, d[7], sizeof(svg_cell_slot) * used, hipMemcpyDeviceToHost) != hipSuccess) {
			svg_set_error("svg_cell_vote_batch: download failed");
			rc = SVG_E_DEVICE;
			break;
		}
		nslots += used;
	}
	for (int i = 0; i < 9; i++) hipFree(d[i]);
	h->device_bytes -= held;
	if (rc) { svg_cell_vote_free(res); return rc; }
	res->n_reads = n;
	res->n_slots = nslots;
	return 0;
}
