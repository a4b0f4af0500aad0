// svg_cell_names.hip -- cellCounts' read-name parsing on the GPU: cellCounts_scan_read_name_str
// (cell-counts.c:1658-1696), the lane number and sample branch of cellCounts_vote_and_add_count
// (:1962-1976) and cellCounts_get_sample_id (:1862-1880) with hamming_dist_ATGC_max1 and
// hamming_dist_ATGC_max1_2p (input-blc.c:1072-1105).  The contract is in include/subread_vote.h.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "svg_cell.h"

#define N_BLOCK 64                   // names per block: one wave (names_parse_kernel takes its minimum by wave shuffles)
#define N_LDS   16384                // bytes of text a block stages (256 a name; a BCL name has about 110)

// a sheet row on the device: the index text as bytes, 8 to a word, character k in byte k % 8 of w[k / 8]
struct SheetRow {
	int32_t lane, sample;
	uint32_t len, dual;
	uint64_t w[4];
};
static_assert(sizeof(SheetRow) == 48 && SVG_CELL_MAX_INDEX == 32, "SheetRow layout");

struct svg_cellnames {
	void *d_rows, *d_lines;
	size_t rows_bytes, lines_bytes;
	uint32_t n_rows, n_lines;
	int n_samples;
	double ms;
};

struct NamesParams {
	const uint8_t *text;             // the batch's text; the allocation is a multiple of 16 bytes
	uint64_t text_bytes;             // rounded up to 16
	const uint64_t *offs;            // the chunk's names
	const uint16_t *lens;
	uint32_t n;
	int bcl, bl, ul;
	const SheetRow *__restrict__ rows;
	uint32_t n_rows;
	const int32_t *__restrict__ lines;
	uint32_t n_lines;
	int32_t *fields, *trimmed, *lane, *sample;
	uint32_t *status, *bc_bases, *bc_xmask, *umi_bases, *umi_xmask;
	unsigned long long *refused;
};

// a name's bytes in LDS or in global memory; beyond its end a name reads as NUL
struct NameText {
	const uint8_t *p;
	uint32_t len;
	__device__ __forceinline__ uint32_t at(uint32_t i) const { return i < len ? p[i] : 0u; }
};

__device__ __forceinline__ bool is_atgcn(uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; }

// a bit for every byte of x that is not zero
__device__ __forceinline__ uint64_t nonzero_bytes(uint64_t x)
{
	return (((x & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | x) & 0x8080808080808080ull;
}

// the mismatches among the first m characters (d: the XOR of the two texts, word by word)
__device__ __forceinline__ int mismatches(const uint64_t d[4], uint32_t m)
{
	int c = 0;
#pragma unroll
	for (uint32_t w = 0; w < 4; w++) {
		const uint32_t k = m > 8u * w ? min(m - 8u * w, 8u) : 0u;
		const uint64_t mask = k == 8u ? ~0ull : (1ull << (8u * k)) - 1ull;
		c += __popcll(nonzero_bytes(d[w]) & mask);
	}
	return c;
}

// `chars` characters from `at` on, packed as svg_packed_reads packs them (A 0, G 1, C 2, T 3; N: 3 and
// the exception bit); 0: a character other than A/C/G/T/N
__device__ __forceinline__ bool pack_text(const NameText &t, uint32_t at, int chars, uint32_t &bases, uint32_t &xmask)
{
	bases = xmask = 0;
	bool ok = true;
	for (int k = 0; k < chars; k++) {
		const uint32_t c = t.p[at + k];
		const uint32_t code = c == 'A' ? 0u : c == 'G' ? 1u : c == 'C' ? 2u : 3u;
		ok = ok && is_atgcn(c);
		bases |= code << (30 - 2 * k);
		xmask |= (uint32_t)(c == 'N') << (31 - k);
	}
	return ok;
}

__device__ __forceinline__ void parse_name(const NamesParams &np, const NameText &t, uint32_t r)
{
	int field = 0, trimmed = 0, lane = -1, sample = -1;
	uint32_t bc = 0, s3 = 0, lp = 0, status = SVG_CELL_NAME_OK, bcb = 0, bcx = 0, umb = 0, umx = 0;
	bool have_lane = false;
	for (uint32_t i = 1; i < t.len; i++) {            // :1662-1683
		const uint32_t c = t.p[i];
		if (c != '|' && !(c == ':' && np.bcl)) continue;
		field++;
		if (field == 1) { trimmed = (int)i; bc = i + 1; }
		else if (field == 3) s3 = i + 1;
		else if (field == 5) {
			lp = i + 1;
			have_lane = true;
			const char *rg = "@RgLater@";
			bool later = true;
			for (uint32_t k = 0; k < 9; k++) later = later && t.at(lp + k) == (uint32_t)rg[k];
			if (later) lp += 9;                            // :1679
			break;
		}
	}
	if (field < 3) status = SVG_CELL_NAME_FEW_FIELDS;
	else if (bc + (uint32_t)(np.bl + np.ul) > t.len) status = SVG_CELL_NAME_PAST_END;
	else {
		const bool bc_ok = pack_text(t, bc, np.bl, bcb, bcx), umi_ok = pack_text(t, bc + (uint32_t)np.bl, np.ul, umb, umx);
		if (!bc_ok || !umi_ok) status = SVG_CELL_NAME_BAD_CHAR;
	}
	if (status) bcb = bcx = umb = umx = 0;
	// the rows are read by every lane at once (no lane leaves the loop), so that their loads are scalar
	uint64_t rd[4] = {0, 0, 0, 0};
	uint32_t run = 0;
	const bool by_sheet = !status && have_lane;
	if (by_sheet) {
		uint32_t no = 0;                               // :1967-1971
		for (uint32_t i = lp + 1; ; i++) {
			const uint32_t c = t.at(i);
			if (c < '0' || c > '9') break;
			no = no * 10u + (c - '0');
		}
		lane = (int)no;
		bool going = true;
#pragma unroll
		for (uint32_t k = 0; k < SVG_CELL_MAX_INDEX; k++) {
			const uint32_t c = t.at(s3 + k);
			going = going && is_atgcn(c);
			if (going) { rd[k / 8] |= (uint64_t)c << (8 * (k % 8)); run = k + 1; }
		}
	}
	bool found = !by_sheet;
	for (uint32_t x = 0; x < np.n_rows; x++) {        // :1864-1878
		const SheetRow &row = np.rows[x];
		if (found || !(row.lane == SVG_CELL_LANE_ALL || row.lane == lane)) continue;
		const uint32_t sl = min(run, row.len);
		const uint64_t d[4] = {rd[0] ^ row.w[0], rd[1] ^ row.w[1], rd[2] ^ row.w[2], rd[3] ^ row.w[3]};
		bool hit;
		if (row.dual) {
			const int p1 = mismatches(d, sl / 2u), p2 = mismatches(d, sl) - p1;
			hit = p1 <= 1 && p2 <= 1;
		} else
			hit = mismatches(d, sl) <= 1;
		if (hit) { sample = row.sample; found = true; }
	}
	if (!status && !have_lane) {                       // :1973-1975
		const char *in = "input#";
		bool is_input = true;
		for (uint32_t k = 0; k < 6; k++) is_input = is_input && t.at(s3 + k) == (uint32_t)in[k];
		if (is_input) {
			const int line = ((int)t.at(s3 + 6) - '0') * 1000 + ((int)t.at(s3 + 7) - '0') * 100 + ((int)t.at(s3 + 8) - '0') * 10 +
			                 ((int)t.at(s3 + 9) - '0') + 1;
			sample = line >= 1 && (uint32_t)line <= np.n_lines ? np.lines[line - 1] : 0;
		}
	}
	np.fields[r] = field; np.trimmed[r] = trimmed; np.lane[r] = lane; np.sample[r] = sample; np.status[r] = status;
	np.bc_bases[2 * r] = bcb; np.bc_bases[2 * r + 1] = 0; np.bc_xmask[r] = bcx;
	np.umi_bases[2 * r] = umb; np.umi_bases[2 * r + 1] = 0; np.umi_xmask[r] = umx;
}

// lane = name.  The block's names lie one behind the other in the text, so the block copies the
// N_LDS bytes from its lowest name on into LDS with 16-byte loads and the lanes scan LDS; a name that
// does not lie wholly in those bytes (long names, or offsets in another order) is scanned in global memory
__global__ void __launch_bounds__(N_BLOCK) names_parse_kernel(NamesParams np)
{
	__shared__ uint4 stage[N_LDS / 16];
	const uint32_t tid = threadIdx.x, r = blockIdx.x * N_BLOCK + tid;
	const bool live = r < np.n;
	const uint64_t off = live ? np.offs[r] : 0;
	const uint32_t len = live ? np.lens[r] : 0;
	unsigned long long first = live ? off : ~0ull;       // the block is one wave: its lowest offset by shuffles
	for (int d = 32; d; d >>= 1) {
		const unsigned long long o = __shfl_xor(first, d);
		first = o < first ? o : first;
	}
	const uint64_t lo = first & ~15ull;
	const uint64_t left = np.text_bytes > lo ? np.text_bytes - lo : 0;
	const uint32_t staged = (uint32_t)(left < (uint64_t)N_LDS ? left : (uint64_t)N_LDS);
	for (uint32_t i = tid * 16u; i < staged; i += N_BLOCK * 16u)
		stage[i / 16u] = *(const uint4 *)(np.text + lo + i);
	__syncthreads();
	unsigned long long bal;
	uint32_t st = 0;
	if (live) {
		NameText t;
		t.len = len;
		if (off + len <= lo + staged) {
			t.p = (const uint8_t *)stage + (uint32_t)(off - lo);
			parse_name(np, t, r);
		} else {
			t.p = np.text + off;
			parse_name(np, t, r);
		}
		st = np.status[r];
	}
	bal = __ballot(st != 0);
	if (np.refused && tid == 0 && bal) atomicAdd(np.refused, (unsigned long long)__popcll(bal));
}

// ---------------------------------------------------------------------------------------------
// host side

static svg_cellnames *cns_get(svg_index *h)
{
	if (!h->cns) h->cns = (svg_cellnames *)calloc(1, sizeof(svg_cellnames));
	if (!h->cns) svg_set_error("out of host memory");
	return h->cns;
}

void svg_cell_names_ws_free(svg_index *h)
{
	if (!h->cns) return;
	hipFree(h->cns->d_rows);
	hipFree(h->cns->d_lines);
	free(h->cns);
	h->cns = NULL;
}

int cell_names_samples(svg_index *h) { return h->cns ? h->cns->n_samples : 0; }

extern "C" int svg_cell_set_samples(svg_index *h, const svg_cell_sample_row *rows, uint64_t n_rows, const int32_t *lines, uint64_t n_lines,
                                    int n_samples)
{
	if (!h || (n_rows && !rows) || (n_lines && !lines)) { svg_set_error("svg_cell_set_samples: NULL argument"); return SVG_E_ARG; }
	const bool any = n_rows || n_lines;
	if (any && (n_samples < 1 || n_samples > SVG_CELL_MAX_SAMPLES)) {
		svg_set_error("svg_cell_set_samples: n_samples %d outside 1..%d", n_samples, SVG_CELL_MAX_SAMPLES);
		return SVG_E_ARG;
	}
	if (n_rows > SVG_CELL_MAX_ROWS || n_lines > SVG_CELL_MAX_ROWS) {
		svg_set_error("svg_cell_set_samples: %llu rows and %llu lines (at most %d)", (unsigned long long)n_rows, (unsigned long long)n_lines, SVG_CELL_MAX_ROWS);
		return SVG_E_ARG;
	}
	SheetRow *img = (SheetRow *)calloc(n_rows ? n_rows : 1, sizeof(SheetRow));
	if (!img) { svg_set_error("out of host memory"); return SVG_E_NOMEM; }
	for (uint64_t i = 0; i < n_rows; i++) {
		const svg_cell_sample_row *q = rows + i;
		const size_t len = q->index ? strnlen(q->index, SVG_CELL_MAX_INDEX + 1) : 0;
		const char *why = NULL;
		if (q->sample_no < 1 || q->sample_no > n_samples) why = "a sample number outside 1..n_samples";
		else if (q->lane < 0) why = "a negative lane";
		else if (!len) why = "an empty index";
		else if (len > SVG_CELL_MAX_INDEX) why = "an index of more than SVG_CELL_MAX_INDEX characters";
		for (size_t k = 0; k < len && !why; k++)
			if (!strchr("ACGT", q->index[k])) why = "an index character other than A/C/G/T";
		if (why) { free(img); svg_set_error("svg_cell_set_samples: row %llu: %s", (unsigned long long)i, why); return SVG_E_ARG; }
		img[i].lane = q->lane; img[i].sample = q->sample_no; img[i].len = (uint32_t)len;
		img[i].dual = len > 12;                        // :664
		for (size_t k = 0; k < len; k++) img[i].w[k / 8] |= (uint64_t)(uint8_t)q->index[k] << (8 * (k % 8));
	}
	for (uint64_t i = 0; i < n_lines; i++)
		if (lines[i] < 0 || lines[i] > n_samples) {
			free(img);
			svg_set_error("svg_cell_set_samples: line %llu: sample number %d outside 0..%d", (unsigned long long)(i + 1), lines[i], n_samples);
			return SVG_E_ARG;
		}
	svg_cellnames *cn = cns_get(h);
	if (!cn) { free(img); return SVG_E_NOMEM; }
	int rc = hipSetDevice(h->device) == hipSuccess ? 0 : SVG_E_DEVICE;
	if (!rc && h->last_pending && hipStreamWaitEvent(h->stream, h->ev_last, 0) != hipSuccess) rc = SVG_E_DEVICE;
	if (!rc && hipStreamSynchronize(h->stream) != hipSuccess) rc = SVG_E_DEVICE;
	if (rc) { free(img); svg_set_error("svg_cell_set_samples: HIP error"); return rc; }
	// the new image first; the old one is replaced only once it is in device memory
	void *d_rows = NULL, *d_lines = NULL;
	const size_t rb = sizeof(SheetRow) * n_rows, lb = 4 * n_lines;
	if (n_rows && !(rc = dmalloc(h, &d_rows, rb)) && hipMemcpy(d_rows, img, rb, hipMemcpyHostToDevice) != hipSuccess) rc = SVG_E_DEVICE;
	if (!rc && n_lines && !(rc = dmalloc(h, &d_lines, lb)) && hipMemcpy(d_lines, lines, lb, hipMemcpyHostToDevice) != hipSuccess) rc = SVG_E_DEVICE;
	free(img);
	if (rc) {
		if (d_rows) { hipFree(d_rows); h->device_bytes -= rb; }
		if (d_lines) { hipFree(d_lines); h->device_bytes -= lb; }
		if (rc == SVG_E_DEVICE) svg_set_error("svg_cell_set_samples: upload failed");
		return rc;
	}
	hipFree(cn->d_rows); hipFree(cn->d_lines);
	h->device_bytes -= cn->rows_bytes + cn->lines_bytes;
	cn->d_rows = d_rows; cn->d_lines = d_lines; cn->rows_bytes = n_rows ? rb : 0; cn->lines_bytes = n_lines ? lb : 0;
	cn->n_rows = (uint32_t)n_rows; cn->n_lines = (uint32_t)n_lines;
	cn->n_samples = any ? n_samples : 0;
	return 0;
}

struct CellNamesRun {
	svg_index *h;
	hipStream_t st;
	int mode, bl, ul;
	uint64_t n, chunk, text_bytes;
	void *d_text, *d_offs, *d_lens, *d_out, *d_refused;
	size_t held;
	hipEvent_t ev[2];
};

static int names_alloc(CellNamesRun *r, void **p, size_t bytes)
{
	int rc = dmalloc(r->h, p, bytes);
	if (!rc) r->held += bytes;
	return rc;
}

void cell_names_end(CellNamesRun *r)
{
	if (!r) return;
	hipFree(r->d_text); hipFree(r->d_offs); hipFree(r->d_lens); hipFree(r->d_out); hipFree(r->d_refused);
	for (int i = 0; i < 2; i++)
		if (r->ev[i]) hipEventDestroy(r->ev[i]);
	r->h->device_bytes -= r->held;
	free(r);
}

// a chunk's output: eleven words a name (fields, trimmed, lane, sample, status, 2 + 1 barcode words, 2 + 1 UMI words)
#define N_OUT_WORDS 11

int cell_names_begin(svg_index *h, const char *who, const svg_reads *names, int mode, int bl, int ul, uint64_t n, uint64_t chunk, hipStream_t st,
                     CellNamesRun **out)
{
	*out = NULL;
	if (!cns_get(h)) return SVG_E_NOMEM;      // (the timing lives there, sheet or no sheet)
	if (mode != SVG_CELL_NAMES_BCL && mode != SVG_CELL_NAMES_FASTQ) { svg_set_error("%s: mode %d", who, mode); return SVG_E_ARG; }
	if (bl < 1 || bl > 16) { svg_set_error("%s: barcode_length %d outside 1..16", who, bl); return SVG_E_ARG; }
	if (ul < 1 || ul > SVG_CELL_MAX_UMI) {
		svg_set_error("%s: umi_length %d outside 1..%d (the caller states it; there is no auto-detection)", who, ul, SVG_CELL_MAX_UMI);
		return SVG_E_ARG;
	}
	if (n && (!names->seq || !names->offsets || !names->lens)) { svg_set_error("%s: NULL name buffer", who); return SVG_E_ARG; }
	uint64_t bytes = 0;
	for (uint64_t i = 0; i < n; i++) {
		const uint64_t e = names->offsets[i] + names->lens[i];
		if (e > bytes) bytes = e;
	}
	CellNamesRun *r = (CellNamesRun *)calloc(1, sizeof *r);
	if (!r) { svg_set_error("out of host memory"); return SVG_E_NOMEM; }
	r->h = h; r->st = st; r->mode = mode; r->bl = bl; r->ul = ul; r->n = n; r->chunk = chunk;
	r->text_bytes = (bytes + 15) & ~15ull;
	int rc;
	if ((rc = names_alloc(r, &r->d_text, r->text_bytes + 16)) || (rc = names_alloc(r, &r->d_offs, 8 * n)) || (rc = names_alloc(r, &r->d_lens, 2 * n)) ||
	    (rc = names_alloc(r, &r->d_out, 4 * (size_t)N_OUT_WORDS * chunk)) || (rc = names_alloc(r, &r->d_refused, 8))) {
		cell_names_end(r);
		return rc;
	}
	if (hipMemsetAsync((char *)r->d_text + (r->text_bytes ? r->text_bytes - 16 : 0), 0, r->text_bytes ? 32 : 16, st) != hipSuccess ||
	    (bytes && hipMemcpyAsync(r->d_text, names->seq, bytes, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    (n && hipMemcpyAsync(r->d_offs, names->offsets, 8 * n, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    (n && hipMemcpyAsync(r->d_lens, names->lens, 2 * n, hipMemcpyHostToDevice, st) != hipSuccess) ||
	    hipMemsetAsync(r->d_refused, 0, 8, st) != hipSuccess) {
		svg_set_error("%s: upload failed", who);
		cell_names_end(r);
		return SVG_E_DEVICE;
	}
	if (h->timing)
		for (int i = 0; i < 2; i++)
			if (hipEventCreate(&r->ev[i]) != hipSuccess) { svg_set_error("%s: hipEventCreate failed", who); cell_names_end(r); return SVG_E_DEVICE; }
	*out = r;
	return 0;
}

void cell_names_view(CellNamesRun *r, CellNamesView *v)
{
	uint32_t *o = (uint32_t *)r->d_out;
	const uint64_t m = r->chunk;
	v->fields = (int32_t *)o; v->trimmed = (int32_t *)(o + m); v->lane = (int32_t *)(o + 2 * m); v->sample = (int32_t *)(o + 3 * m);
	v->status = o + 4 * m; v->bc_bases = o + 5 * m; v->bc_xmask = o + 7 * m; v->umi_bases = o + 8 * m; v->umi_xmask = o + 10 * m;
	v->refused = (unsigned long long *)r->d_refused;
}

// the parse kernel over the chunk's k names from first_read on (asynchronous on the run's stream)
int cell_names_chunk(CellNamesRun *r, uint64_t first_read, uint64_t k)
{
	svg_cellnames *cn = r->h->cns;
	if (!k) return 0;
	if (k > r->chunk) { svg_set_error("svg_cell_names: a chunk of %llu names", (unsigned long long)k); return SVG_E_DEVICE; }
	CellNamesView v;
	cell_names_view(r, &v);
	NamesParams np;
	memset(&np, 0, sizeof np);
	np.text = (const uint8_t *)r->d_text; np.text_bytes = r->text_bytes;
	np.offs = (const uint64_t *)r->d_offs + first_read; np.lens = (const uint16_t *)r->d_lens + first_read;
	np.n = (uint32_t)k; np.bcl = r->mode == SVG_CELL_NAMES_BCL; np.bl = r->bl; np.ul = r->ul;
	if (cn) { np.rows = (const SheetRow *)cn->d_rows; np.n_rows = cn->n_rows; np.lines = (const int32_t *)cn->d_lines; np.n_lines = cn->n_lines; }
	np.fields = (int32_t *)v.fields; np.trimmed = (int32_t *)v.trimmed; np.lane = (int32_t *)v.lane; np.sample = (int32_t *)v.sample;
	np.status = (uint32_t *)v.status; np.bc_bases = (uint32_t *)v.bc_bases; np.bc_xmask = (uint32_t *)v.bc_xmask;
	np.umi_bases = (uint32_t *)v.umi_bases; np.umi_xmask = (uint32_t *)v.umi_xmask;
	np.refused = v.refused;
	if (r->ev[0]) hipEventRecord(r->ev[0], r->st);
	hipLaunchKernelGGL(names_parse_kernel, dim3((unsigned)((k + N_BLOCK - 1) / N_BLOCK)), dim3(N_BLOCK), 0, r->st, np);
	if (r->ev[0]) hipEventRecord(r->ev[1], r->st);
	if (hipGetLastError() != hipSuccess) { svg_set_error("svg_cell_names: launch failed"); return SVG_E_DEVICE; }
	return 0;
}

// the last chunk's kernel time into the handle's sum; waits for the kernel's end event itself (the
// callers have synchronised the stream behind the chunk by then, so the wait is over at once)
void cell_names_time(CellNamesRun *r)
{
	float ms = 0;
	if (!r->ev[0]) return;
	if (hipEventSynchronize(r->ev[1]) == hipSuccess && hipEventElapsedTime(&ms, r->ev[0], r->ev[1]) == hipSuccess) r->h->cns->ms += ms;
}

extern "C" void svg_cell_names_free(svg_cell_names *out)
{
	if (!out) return;
	free(out->fields); free(out->trimmed_len); free(out->lane); free(out->sample_no); free(out->status);
	free((void *)out->barcodes.bases); free((void *)out->barcodes.xmask); free((void *)out->barcodes.lens);
	free((void *)out->umis.bases); free((void *)out->umis.xmask); free((void *)out->umis.lens);
	memset(out, 0, sizeof *out);
}

extern "C" int svg_cell_parse_names(svg_index *h, const svg_reads *names, int mode, int barcode_length, int umi_length, svg_cell_names *out)
{
	if (out) memset(out, 0, sizeof *out);
	if (!h || !names || !out) { svg_set_error("svg_cell_parse_names: NULL argument"); return SVG_E_ARG; }
	if (!cns_get(h)) return SVG_E_NOMEM;
	const uint64_t n = names->n_reads, CH = 1u << 17, m = n < CH ? (n ? n : 1) : CH;
	HIPCHK(hipSetDevice(h->device));
	hipStream_t st = h->stream;
	if (h->last_pending) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));
	CellNamesRun *run = NULL;
	int rc = cell_names_begin(h, "svg_cell_parse_names", names, mode, barcode_length, umi_length, n, m, st, &run);
	if (rc) return rc;
	const size_t q = n ? n : 1;
	uint32_t *bcb = (uint32_t *)calloc(2 * q, 4), *bcx = (uint32_t *)calloc(q, 4), *umb = (uint32_t *)calloc(2 * q, 4), *umx = (uint32_t *)calloc(q, 4);
	uint16_t *bl = (uint16_t *)malloc(2 * q), *ul = (uint16_t *)malloc(2 * q);
	out->fields = (int32_t *)malloc(4 * q); out->trimmed_len = (int32_t *)malloc(4 * q); out->lane = (int32_t *)malloc(4 * q);
	out->sample_no = (int32_t *)malloc(4 * q); out->status = (uint32_t *)malloc(4 * q);
	out->barcodes.bases = bcb; out->barcodes.xmask = bcx; out->barcodes.lens = bl; out->barcodes.stride = SVG_CELL_NAME_STRIDE;
	out->umis.bases = umb; out->umis.xmask = umx; out->umis.lens = ul; out->umis.stride = SVG_CELL_NAME_STRIDE;
	if (!bcb || !bcx || !umb || !umx || !bl || !ul || !out->fields || !out->trimmed_len || !out->lane || !out->sample_no || !out->status) {
		svg_set_error("out of host memory");
		rc = SVG_E_NOMEM;
	}
	CellNamesView v;
	cell_names_view(run, &v);
	for (uint64_t o = 0; o < n && !rc; o += m) {
		const uint64_t k = n - o < m ? n - o : m;
		if ((rc = cell_names_chunk(run, o, k))) break;
		if (hipMemcpyAsync(out->fields + o, v.fields, 4 * k, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipMemcpyAsync(out->trimmed_len + o, v.trimmed, 4 * k, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipMemcpyAsync(out->lane + o, v.lane, 4 * k, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipMemcpyAsync(out->sample_no + o, v.sample, 4 * k, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipMemcpyAsync(out->status + o, v.status, 4 * k, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipMemcpyAsync(bcb + 2 * o, v.bc_bases, 8 * k, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipMemcpyAsync(bcx + o, v.bc_xmask, 4 * k, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipMemcpyAsync(umb + 2 * o, v.umi_bases, 8 * k, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipMemcpyAsync(umx + o, v.umi_xmask, 4 * k, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipStreamSynchronize(st) != hipSuccess) {
			svg_set_error("svg_cell_parse_names: HIP error %s", hipGetErrorString(hipGetLastError()));
			rc = SVG_E_DEVICE;
			break;
		}
		cell_names_time(run);
	}
	unsigned long long refused = 0;
	if (!rc && (hipMemcpyAsync(&refused, v.refused, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
		svg_set_error("svg_cell_parse_names: HIP error");
		rc = SVG_E_DEVICE;
	}
	if (rc) hipStreamSynchronize(st);
	cell_names_end(run);
	if (rc) { svg_cell_names_free(out); return rc; }
	for (uint64_t i = 0; i < n; i++) { bl[i] = (uint16_t)barcode_length; ul[i] = (uint16_t)umi_length; }
	out->barcodes.n_reads = out->umis.n_reads = out->n_reads = n;
	out->refused = refused;
	return 0;
}

extern "C" int svg_cell_names_timing(svg_index *h, double *ms)
{
	if (!h || !ms) { svg_set_error("svg_cell_names_timing: NULL argument"); return SVG_E_ARG; }
	*ms = h->cns ? h->cns->ms : 0;
	if (h->cns) h->cns->ms = 0;
	return 0;
}
