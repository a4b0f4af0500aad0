// svg_keys.hip -- equal-key runs of arbitrary subread keys (include/subread_vote.h svg_probe_keys*).
//
// cellCounts does not call gehash_go_X: its voting first lists, for every subread of a read,
// the bucket-local run of items whose key equals the subread's (prefill_votes,
// cell-counts.c:432-491), and votes over those lists itself.  That lookup is the probe half of
// the vote path (a3-a4) with a different widening: binary search of (short)(key / buckets) in
// the bucket's keys (sorted-hashtable.c's layout), then forward / backward steps of imax/4,
// /3, /3 ... that only land on equal keys, then single steps to the run's ends.
//
// In a bucket whose keys are sorted, those steps find exactly the whole equal-key run -- the
// run the vote path's probe images already hold:
//   bucket code (full indexes, build_bcode): one random 32-byte sector per key gives the run's
//     bucket-local bounds directly (count byte 255 = not coded: unsorted or > 169 items);
//   key hash (gapped / small indexes, build_khash): one random sector gives the record
//     (mid item, fwd, bwd) of the run, and the bucket's first item turns it bucket-local; a
//     bucket whose keys are not sorted (DevIndex::ksorted) takes the literal search instead.
// The literal search (one thread per key over the resident bounds + i16 keys) answers
// everything else; SVG_KEYS_LITERAL=1 forces it (A/B and tests).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "subread_vote.h"
#include "svg_internal.h"
#include "svg_device.h"

#include "svg_keylookup.h"

struct KeyParams {
	KeyTable t;
	const uint32_t *in;
	uint64_t n;
	uint32_t *first, *count;
};

template <int IMG>
__global__ void __launch_bounds__(256) probe_keys_kernel(KeyParams kp)
{
	for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < kp.n; t += (uint64_t)gridDim.x * 256u) {
		uint32_t f, c;
		key_run<IMG>(kp.t, kp.in[t], f, c);
		kp.first[t] = f;
		kp.count[t] = c;
	}
}

static svg_index *key_block(svg_index *h, int block)
{
	if (!h) { svg_set_error("svg_probe_keys: no index"); return NULL; }
	if (block < 0 || block >= (h->nblocks > 0 ? h->nblocks : 1)) {
		svg_set_error("svg_probe_keys: block %d of an index with %d block(s)", block, h->nblocks > 0 ? h->nblocks : 1);
		return NULL;
	}
	return block ? h->blk[block] : h;
}

static int launch_keys(svg_index *h, svg_index *bk, const uint32_t *keys, uint64_t n, uint32_t *first, uint32_t *count,
                       hipStream_t st)
{
	if (n == 0) return 0;
	KeyParams kp;
	kp.t = key_table(bk);
	kp.in = keys;
	kp.n = n;
	kp.first = first;
	kp.count = count;
	uint64_t blocks = (n + 255) / 256, bmax = (uint64_t)h->n_cu * 16;
	if (blocks > bmax) blocks = bmax;
	const int img = key_image(bk);
	if (img == KEYS_CODE) hipLaunchKernelGGL(probe_keys_kernel<KEYS_CODE>, dim3((unsigned)blocks), dim3(256), 0, st, kp);
	else if (img == KEYS_KHASH) hipLaunchKernelGGL(probe_keys_kernel<KEYS_KHASH>, dim3((unsigned)blocks), dim3(256), 0, st, kp);
	else hipLaunchKernelGGL(probe_keys_kernel<KEYS_LITERAL>, dim3((unsigned)blocks), dim3(256), 0, st, kp);
	HIPCHK(hipGetLastError());
	return 0;
}

extern "C" int svg_probe_keys_device(svg_index *h, int block, const uint32_t *keys, uint64_t n, uint32_t *first,
                                     uint32_t *count, void *hip_stream)
{
	svg_index *bk = key_block(h, block);
	if (!bk) return SVG_E_ARG;
	if (n && (!keys || !first || !count)) { svg_set_error("svg_probe_keys_device: NULL buffer"); return SVG_E_ARG; }
	HIPCHK(hipSetDevice(h->device));
	hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->stream;
	// the handle's earlier work first (its buffers are not touched, but the index may still be
	// under construction on the handle's stream)
	if (st != h->stream) {
		hipEvent_t ev;
		HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
		HIPCHK(hipEventRecord(ev, h->stream));
		HIPCHK(hipStreamWaitEvent(st, ev, 0));
		HIPCHK(hipEventDestroy(ev));
	}
	return launch_keys(h, bk, keys, n, first, count, st);
}

extern "C" int svg_probe_keys(svg_index *h, int block, const uint32_t *keys, uint64_t n, uint32_t *first, uint32_t *count)
{
	svg_index *bk = key_block(h, block);
	if (!bk) return SVG_E_ARG;
	if (n == 0) return 0;
	if (!keys || !first || !count) { svg_set_error("svg_probe_keys: NULL buffer"); return SVG_E_ARG; }
	HIPCHK(hipSetDevice(h->device));
	const uint64_t CH = 16u << 20;   // keys per round trip (192 MB of device buffers)
	const uint64_t m = n < CH ? n : CH;
	void *d = NULL;
	if (dmalloc(h, &d, 12 * m)) return SVG_E_NOMEM;
	uint32_t *dk = (uint32_t *)d, *df = dk + m, *dc = df + m;
	int rc = 0;
	for (uint64_t o = 0; o < n && !rc; o += m) {
		const uint64_t k = n - o < m ? n - o : m;
		if (hipMemcpyAsync(dk, keys + o, 4 * k, hipMemcpyHostToDevice, h->stream) != hipSuccess) { rc = SVG_E_DEVICE; break; }
		if ((rc = launch_keys(h, bk, dk, k, df, dc, h->stream))) break;
		if (hipMemcpyAsync(first + o, df, 4 * k, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
		    hipMemcpyAsync(count + o, dc, 4 * k, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
		    hipStreamSynchronize(h->stream) != hipSuccess) { rc = SVG_E_DEVICE; break; }
	}
	if (rc == SVG_E_DEVICE) svg_set_error("svg_probe_keys: HIP error %s", hipGetErrorString(hipGetLastError()));
	hipFree(d);
	h->device_bytes -= 12 * m;
	return rc;
}
