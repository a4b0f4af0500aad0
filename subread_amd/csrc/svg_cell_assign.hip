// svg_cell_assign.hip -- cellCounts' gene assignment and cell-barcode lookup on the GPU, behind
// svg_cell_align.hip's records: cellCounts_write_read_in_batch_bin (cell-counts.c:2061-2088) with
// cellCounts_find_hits_for_mapped_section (:1575-1654), cellCounts_summarize_entrez_hits
// (:2039-2059), the rule of :1982 and cellCounts_get_cellbarcode_no (:1701-1768).  The contract is
// in include/subread_vote.h; the tables come from svg_cell_annot.c.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "svg_cell.h"
#include "svg_cell_annot.h"

#define A_BUCKET SVG_CELL_REV_BUCKET
#define A_GENES  SVG_CELL_MAX_GENES
#define A_COUNT  100000000           // a CIGAR count saturates here (a caller's record; the library's own sum to <= 160)

struct AssignTables {
	const uint32_t *fstart, *fend;
	const int32_t *fgene;
	const uint8_t *fstrand;
	const uint32_t *bend, *bmin, *bmax;
	const uint32_t *chro_len, *chro_bend, *rev_first, *rev;
	const uint32_t *chr_end;
	uint32_t n_chr;
	int padding, have, allow_multi;
};

struct BarcodeTables {
	const uint32_t *code, *frow, *srow, *fent, *sent;
	uint32_t n, length;
};

struct svg_cellassign {
	void *d_annot;            // one allocation: the arrays of AssignTables
	size_t annot_bytes;
	AssignTables at;
	void *d_bcodes;           // one allocation: the arrays of BarcodeTables
	size_t bcodes_bytes;
	BarcodeTables bt;
	double ms[3];             // assign, barcode, scan + compact
};

struct AssignParams {
	AssignTables at;
	const svg_cell_aln *recs;
	uint32_t n;               // records
	svg_cell_hit *hits;       // [n]
	int32_t *stage;           // [n][A_GENES]
	int32_t *genes;           // compacted
	uint64_t gene_base;
	uint64_t *total;          // the chunk's gene count
	uint32_t *overflow;       // alignments over more than A_GENES distinct genes
};

struct BarcodeParams {
	BarcodeTables bt;
	const uint32_t *bases, *xmask;
	const uint64_t *starts;
	uint64_t stride, base0;
	uint32_t n;
	int32_t *out;
};

// one M section [b, e] of contig c (:1575-1654): the distinct genes go to st[0 .. cnt)
__device__ __forceinline__ void assign_section(const AssignTables &t, uint32_t c, int b, int e, int neg, int32_t *st, uint32_t &cnt,
                                               uint32_t &over)
{
	if (b < 0 || e < b) return;       // (no record of svg_cell_align_batch: a count that overflowed an int)
	int s = b / (int)A_BUCKET, en = (1 + e) / (int)A_BUCKET;
	const int top = (int)(t.chro_len[c] / A_BUCKET);
	s = min(s, top);                  // :1602
	en = min(en, top + 1);            // :1603
	const uint32_t *rt = t.rev + t.rev_first[c];
	uint32_t ss = 0xffffffffu;
	while (s <= en) {                 // :1605-1609
		ss = rt[s];
		if (ss < 0xffffff00u) break;
		s++;
	}
	if (ss > 0xffffff00u) return;     // :1611
	const uint32_t last = t.chro_bend[c];
	for (uint32_t blk = ss; blk < last; blk++) {
		if ((int64_t)t.bmin[blk] > (int64_t)e) break;       // :1616
		if ((int64_t)t.bmax[blk] < (int64_t)b) continue;    // :1617
		const uint32_t i1 = t.bend[blk];
		for (uint32_t it = blk ? t.bend[blk - 1] : 0u; it < i1; it++) {
			if ((int64_t)t.fend[it] < (int64_t)b) continue;     // :1626
			if ((int64_t)t.fstart[it] > (int64_t)e) break;      // :1627
			if ((int)t.fstrand[it] != neg) continue;            // :1631
			const int32_t g = t.fgene[it];
			// cellCounts_summarize_entrez_hits (:2051-2056): first seen first
			uint32_t k = 0;
			while (k < cnt && st[k] != g) k++;
			if (k < cnt) continue;
			if (cnt < (uint32_t)A_GENES) st[cnt++] = g;
			else over = 1;
		}
	}
}

// thread = alignment record: locate_gene_position, the head soft clip, the CIGAR walk
__global__ void __launch_bounds__(256) assign_kernel(AssignParams ap)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= ap.n) return;
	const AssignTables &t = ap.at;
	const svg_cell_aln *rec = ap.recs + i;
	svg_cell_hit h;
	h.contig = -1; h.chro_pos = 0; h.nhits = 0; h._pad = 0; h.first_gene = 0;
	// locate_gene_position_max with rl = 0 and no cut lengths (gene-algorithms.c:441-511)
	const uint32_t linear = rec->position + 1u;
	int lo = 0, hi = (int)t.n_chr;
	while (hi > lo + 1) {
		const int mid = (lo + hi) / 2;
		if (t.chr_end[mid] > linear) hi = mid; else lo = mid + 1;
	}
	int n = max(lo - 2, 0), pos = 0, c = -1;
	for (; n < (int)t.n_chr; n++)
		if (t.chr_end[n] > linear) {
			pos = n == 0 ? (int)linear : (int)(linear - t.chr_end[n - 1]);
			if (linear > t.chr_end[n] + 15u - (uint32_t)t.padding) break;    // :476
			if (pos < t.padding) break;                                     // :495-497
			pos -= t.padding;
			c = n;
			break;
		}
	if (c >= 0) {
		const char *cg = rec->cigar;
		// get_soft_clipping_length (core.c:1232-1247): the count before a first operation S
		int v = 0, q = 0;
		while (q < SVG_CELL_CIGAR && cg[q] >= '0' && cg[q] <= '9') { v = min(v * 10 + (cg[q] - '0'), A_COUNT); q++; }
		if (q < SVG_CELL_CIGAR && cg[q] == 'S') pos += v;
		h.contig = c;
		h.chro_pos = pos;
		if (t.have) {
			int32_t *st = ap.stage + (size_t)i * A_GENES;
			uint32_t cnt = 0, over = 0;
			const int neg = (rec->flags & 16) ? 1 : 0;
			int tmpi = 0;
			for (q = 0; q < SVG_CELL_CIGAR; q++) {    // :2074-2083: the cursor stays at chro_pos
				const int ch = cg[q];
				if (!ch) break;
				if (ch >= '0' && ch <= '9') tmpi = min(10 * tmpi + (ch - '0'), A_COUNT);
				else {
					if (ch == 'M') assign_section(t, (uint32_t)c, pos, pos + tmpi, neg, st, cnt, over);
					tmpi = 0;
				}
			}
			if (cnt > 1 && !t.allow_multi) cnt = 0;   // :1982
			else if (over) { atomicAdd(ap.overflow, 1u); cnt = 0; }
			h.nhits = cnt;
		}
	}
	ap.hits[i] = h;
}

// hits[i].first_gene = gene_base + (genes of the chunk's records before i) for a record with genes
__global__ void __launch_bounds__(1024) assign_scan_kernel(AssignParams ap)
{
	__shared__ uint32_t part[1024];
	const uint32_t tid = threadIdx.x, n = ap.n, per = (n + 1023u) / 1024u;
	const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
	uint32_t sum = 0;
	for (uint32_t r = lo; r < hi; r++) sum += ap.hits[r].nhits;
	part[tid] = sum;
	__syncthreads();
	for (uint32_t d = 1; d < 1024u; d <<= 1) {
		const uint32_t v = tid >= d ? part[tid - d] : 0u;
		__syncthreads();
		part[tid] += v;
		__syncthreads();
	}
	uint64_t at = ap.gene_base + (part[tid] - sum);
	for (uint32_t r = lo; r < hi; r++) {
		const uint32_t k = ap.hits[r].nhits;
		if (k) ap.hits[r].first_gene = at;
		at += k;
	}
	if (tid == 1023u) *ap.total = part[1023];
}

// thread = (record, k): the record's k-th gene to its place
__global__ void __launch_bounds__(256) assign_compact_kernel(AssignParams ap)
{
	const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (t >= (uint64_t)ap.n * A_GENES) return;
	const uint32_t i = (uint32_t)(t / A_GENES), k = (uint32_t)(t % A_GENES);
	const svg_cell_hit *h = ap.hits + i;
	if (k >= h->nhits) return;
	ap.genes[h->first_gene - ap.gene_base + k] = ap.stage[t];
}

// base k of a packed stream and its exception bit (subread_vote.h: svg_packed_reads)
__device__ __forceinline__ uint32_t packed_base(const uint32_t *bases, uint64_t k) { return (bases[k >> 4] >> (30u - 2u * (uint32_t)(k & 15u))) & 3u; }
__device__ __forceinline__ uint32_t packed_exc(const uint32_t *xmask, uint64_t k) { return (xmask[k >> 5] >> (31u - (uint32_t)(k & 31u))) & 1u; }

// thread = read: cellCounts_get_cellbarcode_no (:1701-1768)
__global__ void __launch_bounds__(256) barcode_kernel(BarcodeParams bp)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r >= bp.n) return;
	const BarcodeTables &t = bp.bt;
	const uint64_t base = bp.starts ? bp.starts[r] : bp.base0 + (uint64_t)r * bp.stride;
	const uint32_t L = t.length, half = L / 2u;
	uint32_t code = 0, exc = 0, fk = 0, sk = 0, fbad = 0, sbad = 0;   // exc: bit 2i for an N at position i
	for (uint32_t k = 0; k < L; k++) {
		const uint32_t b = packed_base(bp.bases, base + k), x = bp.xmask ? packed_exc(bp.xmask, base + k) : 0u;
		code |= b << (2u * k);
		exc |= x << (2u * k);
		if (k / 2u < half) {
			if (k & 1u) { sk |= b << (k / 2u * 2u); sbad |= x; }
			else { fk |= b << (k / 2u * 2u); fbad |= x; }
		}
	}
	const uint32_t chars = L == 16u ? 0x55555555u : ((1u << (2u * L)) - 1u) & 0x55555555u;
	int32_t ans = -1, first1 = -1;
	// the F row: the exact entry wherever it stands (:1721-1730), else the row's first entry at distance 1
	if (!fbad)
		for (uint32_t q = t.frow[fk]; q < t.frow[fk + 1]; q++) {
			const uint32_t w = t.fent[q], d = code ^ t.code[w];
			const int dist = __popc(((d | (d >> 1)) | exc) & chars);   // an N is a mismatch (is_ATGC takes it, input-blc.c:1054)
			if (dist == 0) { ans = (int32_t)w; break; }
			if (dist == 1 && first1 < 0) first1 = (int32_t)w;
		}
	if (ans < 0) ans = first1;
	if (ans < 0 && !sbad)
		for (uint32_t q = t.srow[sk]; q < t.srow[sk + 1]; q++) {
			const uint32_t w = t.sent[q], d = code ^ t.code[w];
			if (__popc(((d | (d >> 1)) | exc) & chars) == 1) { ans = (int32_t)w; break; }
		}
	bp.out[r] = ans;
}

// ---------------------------------------------------------------------------------------------
// host side

static svg_cellassign *cas_get(svg_index *h)
{
	if (!h->cas) h->cas = (svg_cellassign *)calloc(1, sizeof(svg_cellassign));
	if (!h->cas) svg_set_error("out of host memory");
	return h->cas;
}

void svg_cell_assign_ws_free(svg_index *h)
{
	if (!h->cas) return;
	hipFree(h->cas->d_annot);
	hipFree(h->cas->d_bcodes);
	free(h->cas);
	h->cas = NULL;
}

static int quiesce(svg_index *h)
{
	HIPCHK(hipSetDevice(h->device));
	if (h->last_pending) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_last, 0));
	HIPCHK(hipStreamSynchronize(h->stream));
	return 0;
}

// the arrays back to back in one allocation, each at a multiple of 16 bytes
struct Piece { const void *src; size_t bytes; const void **dst; };

static int upload_pieces(svg_index *h, Piece *pc, int n, void **d_out, size_t *bytes_out)
{
	size_t total = 0;
	for (int i = 0; i < n; i++) total += (pc[i].bytes + 15) & ~(size_t)15;
	void *d = NULL;
	int rc = dmalloc(h, &d, total);
	if (rc) return rc;
	size_t at = 0;
	for (int i = 0; i < n; i++) {
		if (pc[i].bytes && hipMemcpy((char *)d + at, pc[i].src, pc[i].bytes, hipMemcpyHostToDevice) != hipSuccess) {
			hipFree(d);
			h->device_bytes -= total;
			svg_set_error("upload failed: %s", hipGetErrorString(hipGetLastError()));
			return SVG_E_DEVICE;
		}
		*pc[i].dst = (char *)d + at;
		at += (pc[i].bytes + 15) & ~(size_t)15;
	}
	*d_out = d;
	*bytes_out = total;
	return 0;
}

extern "C" int svg_cell_set_annotation(svg_index *h, const svg_cell_feature *features, uint64_t n, int allow_multi_overlap)
{
	if (!h || (n && !features)) { svg_set_error("svg_cell_set_annotation: NULL argument"); return SVG_E_ARG; }
	if (h->nblocks > 1) {
		svg_set_error("svg_cell_set_annotation: an index of %d blocks (cellCounts takes a one-block index)", h->nblocks);
		return SVG_E_UNSUPPORTED;
	}
	svg_cellassign *ca = cas_get(h);
	if (!ca) return SVG_E_NOMEM;
	svg_cell_annot a;
	memset(&a, 0, sizeof a);
	char why[256];
	int rc;
	if (n && (rc = svg_cell_annot_build(features, n, h->host.chr_end, h->host.n_chr, h->host.padding, &a, why, sizeof why))) {
		svg_set_error("svg_cell_set_annotation: %s", why);
		return rc;
	}
	if ((rc = quiesce(h))) { svg_cell_annot_free(&a); return rc; }
	// the new image first; the planes and the old image are replaced only once it is in HBM
	AssignTables t;
	memset(&t, 0, sizeof t);
	void *d_new = NULL;
	size_t new_bytes = 0;
	if (n) {
	Piece pc[] = {
		{a.start, 4 * (size_t)a.n_features, (const void **)&t.fstart}, {a.end, 4 * (size_t)a.n_features, (const void **)&t.fend},
		{a.gene, 4 * (size_t)a.n_features, (const void **)&t.fgene}, {a.strand, (size_t)a.n_features, (const void **)&t.fstrand},
		{a.block_end, 4 * (size_t)a.n_blocks, (const void **)&t.bend}, {a.block_min, 4 * (size_t)a.n_blocks, (const void **)&t.bmin},
		{a.block_max, 4 * (size_t)a.n_blocks, (const void **)&t.bmax}, {a.chro_len, 4 * (size_t)a.n_contigs, (const void **)&t.chro_len},
		{a.chro_block_end, 4 * (size_t)a.n_contigs, (const void **)&t.chro_bend}, {a.rev_first, 4 * (size_t)a.n_contigs, (const void **)&t.rev_first},
		{a.rev, 4 * (size_t)a.rev_words, (const void **)&t.rev},
	};
	rc = upload_pieces(h, pc, (int)(sizeof pc / sizeof pc[0]), &d_new, &new_bytes);
	if (rc) { svg_cell_annot_free(&a); return rc; }
	t.have = 1;
	t.allow_multi = allow_multi_overlap != 0;
	}
	rc = svg_cell_set_exons(h, a.exon_start, a.exon_stop, n);
	svg_cell_annot_free(&a);
	if (rc) { if (d_new) { hipFree(d_new); h->device_bytes -= new_bytes; } return rc; }
	if (ca->d_annot) { hipFree(ca->d_annot); h->device_bytes -= ca->annot_bytes; }
	ca->d_annot = d_new;
	ca->annot_bytes = new_bytes;
	ca->at = t;
	return 0;
}

extern "C" int svg_cell_set_barcodes(svg_index *h, const char *const *barcodes, uint64_t n, int length)
{
	if (!h || (n && !barcodes)) { svg_set_error("svg_cell_set_barcodes: NULL argument"); return SVG_E_ARG; }
	svg_cellassign *ca = cas_get(h);
	if (!ca) return SVG_E_NOMEM;
	svg_cell_bcodes b;
	memset(&b, 0, sizeof b);
	char why[256];
	int rc;
	if (n && (rc = svg_cell_bcodes_build(barcodes, n, length, &b, why, sizeof why))) {
		svg_set_error("svg_cell_set_barcodes: %s", why);
		return rc;
	}
	if ((rc = quiesce(h))) { svg_cell_bcodes_free(&b); return rc; }
	if (ca->d_bcodes) { hipFree(ca->d_bcodes); ca->d_bcodes = NULL; h->device_bytes -= ca->bcodes_bytes; ca->bcodes_bytes = 0; }
	memset(&ca->bt, 0, sizeof ca->bt);
	if (!n) return 0;
	BarcodeTables &t = ca->bt;
	Piece pc[] = {
		{b.code, 4 * (size_t)b.n, (const void **)&t.code}, {b.frow, 4 * ((size_t)b.rows + 1), (const void **)&t.frow},
		{b.srow, 4 * ((size_t)b.rows + 1), (const void **)&t.srow}, {b.fent, 4 * (size_t)b.n, (const void **)&t.fent},
		{b.sent, 4 * (size_t)b.n, (const void **)&t.sent},
	};
	rc = upload_pieces(h, pc, (int)(sizeof pc / sizeof pc[0]), &ca->d_bcodes, &ca->bcodes_bytes);
	const uint32_t nn = b.n, ll = b.length;
	svg_cell_bcodes_free(&b);
	if (rc) { memset(&ca->bt, 0, sizeof ca->bt); return rc; }
	t.n = nn;
	t.length = ll;
	return 0;
}

struct CellAssignRun {
	svg_index *h;
	hipStream_t st;
	uint64_t n, cap_recs;     // reads of the batch; records the chunk buffers hold
	int have_bc;
	void *d_bases, *d_xmask, *d_starts, *d_bc, *d_hits, *d_stage, *d_genes, *d_total;
	uint64_t stride;
	size_t held;
	svg_cell_hit *hits;       // host arrays, grown chunk by chunk
	int32_t *genes, *bc;
	uint64_t n_hits, cap_hits, n_genes, cap_genes;
	hipEvent_t ev[5];
	bool quiet;               // svg_cell_count_batch without a result: the host arrays stay empty
	bool device_bc;           // the chunks' barcodes come from device memory (cell_assign_chunk)
	uint64_t chunk_gene_base, chunk_genes;   // of the last chunk (cell_assign_view)
};

static void run_free(CellAssignRun *r)
{
	void *d[] = {r->d_bases, r->d_xmask, r->d_starts, r->d_bc, r->d_hits, r->d_stage, r->d_genes, r->d_total};
	for (size_t i = 0; i < sizeof d / sizeof d[0]; i++) hipFree(d[i]);
	for (int i = 0; i < 5; i++)
		if (r->ev[i]) hipEventDestroy(r->ev[i]);
	r->h->device_bytes -= r->held;
	free(r->hits); free(r->genes); free(r->bc);
	free(r);
}

static int run_alloc(CellAssignRun *r, void **p, size_t bytes)
{
	int rc = dmalloc(r->h, p, bytes);
	if (!rc) r->held += bytes;
	return rc;
}

// the device buffers of a run over chunks of at most cap_recs records
static int run_buffers(CellAssignRun *r, uint64_t cap_recs)
{
	int rc;
	r->cap_recs = cap_recs;
	if ((rc = run_alloc(r, &r->d_hits, sizeof(svg_cell_hit) * cap_recs)) || (rc = run_alloc(r, &r->d_stage, 4 * (size_t)A_GENES * cap_recs)) ||
	    (rc = run_alloc(r, &r->d_genes, 4 * (size_t)A_GENES * cap_recs)) || (rc = run_alloc(r, &r->d_total, 16)))
		return rc;
	if (r->h->timing)
		for (int i = 0; i < 5; i++)
			if (hipEventCreate(&r->ev[i]) != hipSuccess) { svg_set_error("svg_cell_assign: hipEventCreate failed"); return SVG_E_DEVICE; }
	return 0;
}

int cell_assign_barcode_length(svg_index *h) { return h->cas && h->cas->bt.n ? (int)h->cas->bt.length : 0; }

int cell_assign_begin(svg_index *h, const svg_packed_reads *bc, uint64_t n, uint64_t chunk, int max_report, hipStream_t st, CellAssignRun **out, bool quiet,
                      bool device_bc)
{
	*out = NULL;
	svg_cellassign *ca = cas_get(h);
	if (!ca) return SVG_E_NOMEM;
	CellAssignRun *r = (CellAssignRun *)calloc(1, sizeof *r);
	if (!r) { svg_set_error("out of host memory"); return SVG_E_NOMEM; }
	r->h = h; r->st = st; r->n = n; r->quiet = quiet;
	r->have_bc = (bc || device_bc) && ca->bt.n;
	r->device_bc = device_bc;
	int rc = run_buffers(r, chunk * (uint64_t)max_report);
	if (!quiet) r->bc = (int32_t *)malloc(4 * (n ? n : 1));
	if (!rc && !quiet && !r->bc) { svg_set_error("out of host memory"); rc = SVG_E_NOMEM; }
	if (!rc && r->have_bc && device_bc) rc = run_alloc(r, &r->d_bc, 4 * chunk);
	if (!rc && r->have_bc && !device_bc) {
		const uint32_t L = ca->bt.length;
		uint64_t nbases = 0;
		if (!bc->bases || !bc->lens) { svg_set_error("svg_cell_assign_batch: NULL barcode buffer"); rc = SVG_E_ARG; }
		for (uint64_t i = 0; i < n && !rc; i++) {
			if (bc->lens[i] != L) {
				svg_set_error("svg_cell_assign_batch: barcode %llu has %d bases (the whitelist's have %u)", (unsigned long long)i, (int)bc->lens[i], L);
				rc = SVG_E_ARG;
			} else if (!bc->starts && L > bc->stride) {
				svg_set_error("svg_cell_assign_batch: barcode %llu is longer than the stride", (unsigned long long)i);
				rc = SVG_E_ARG;
			}
			const uint64_t e = (bc->starts ? bc->starts[i] : i * bc->stride) + L;
			if (e > nbases) nbases = e;
		}
		const size_t bw = (size_t)((nbases + 15) / 16) * 4, xw = bc->xmask ? (size_t)((nbases + 31) / 32) * 4 : 0;
		r->stride = bc->stride;
		if (!rc) rc = run_alloc(r, &r->d_bases, bw);
		if (!rc && xw) rc = run_alloc(r, &r->d_xmask, xw);
		if (!rc && bc->starts) rc = run_alloc(r, &r->d_starts, 8 * n);
		if (!rc) rc = run_alloc(r, &r->d_bc, 4 * chunk);
		if (!rc && (hipMemcpyAsync(r->d_bases, bc->bases, bw, hipMemcpyHostToDevice, st) != hipSuccess ||
		            (xw && hipMemcpyAsync(r->d_xmask, bc->xmask, xw, hipMemcpyHostToDevice, st) != hipSuccess) ||
		            (bc->starts && hipMemcpyAsync(r->d_starts, bc->starts, 8 * n, hipMemcpyHostToDevice, st) != hipSuccess))) {
			svg_set_error("svg_cell_assign_batch: upload failed");
			rc = SVG_E_DEVICE;
		}
	}
	if (rc) { run_free(r); return rc; }
	*out = r;
	return 0;
}

// the records at d_recs (device) -> the run's host arrays
static int run_records(CellAssignRun *r, const svg_cell_aln *d_recs, uint64_t used, int with_barcode_event)
{
	svg_index *h = r->h;
	svg_cellassign *ca = h->cas;
	hipStream_t st = r->st;
	if (!used) return 0;
	AssignParams ap;
	memset(&ap, 0, sizeof ap);
	ap.at = ca->at;
	ap.at.chr_end = h->dix.chr_end;
	ap.at.n_chr = h->dix.n_chr;
	ap.at.padding = h->dix.padding;
	ap.recs = d_recs;
	ap.n = (uint32_t)used;
	ap.hits = (svg_cell_hit *)r->d_hits;
	ap.stage = (int32_t *)r->d_stage;
	ap.genes = (int32_t *)r->d_genes;
	ap.gene_base = r->n_genes;
	ap.total = (uint64_t *)r->d_total;
	ap.overflow = (uint32_t *)r->d_total + 2;
	if (hipMemsetAsync(r->d_total, 0, 16, st) != hipSuccess) { svg_set_error("svg_cell_assign: HIP error"); return SVG_E_DEVICE; }
	// (events: 0 .. 1 the barcode kernel, recorded by cell_assign_chunk; 4 .. 2 the assign kernel; 2 .. 3 scan + compact)
	if (r->ev[0]) hipEventRecord(r->ev[4], st);
	hipLaunchKernelGGL(assign_kernel, dim3((unsigned)((used + 255) / 256)), dim3(256), 0, st, ap);
	if (r->ev[0]) hipEventRecord(r->ev[2], st);
	hipLaunchKernelGGL(assign_scan_kernel, dim3(1), dim3(1024), 0, st, ap);
	hipLaunchKernelGGL(assign_compact_kernel, dim3((unsigned)((used * A_GENES + 255) / 256)), dim3(256), 0, st, ap);
	if (r->ev[0]) hipEventRecord(r->ev[3], st);
	uint64_t tot[2] = {0, 0};
	if (!r->quiet && r->n_hits + used > r->cap_hits) {
		const uint64_t cap = (r->n_hits + used) * 2;
		svg_cell_hit *g = (svg_cell_hit *)realloc(r->hits, sizeof(svg_cell_hit) * cap);
		if (!g) { svg_set_error("out of host memory"); return SVG_E_NOMEM; }
		r->hits = g; r->cap_hits = cap;
	}
	if (hipGetLastError() != hipSuccess ||
	    (!r->quiet && hipMemcpyAsync(r->hits + r->n_hits, r->d_hits, sizeof(svg_cell_hit) * used, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    hipMemcpyAsync(tot, r->d_total, 16, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
		svg_set_error("svg_cell_assign: HIP error %s", hipGetErrorString(hipGetLastError()));
		return SVG_E_DEVICE;
	}
	if (tot[1]) {
		svg_set_error("svg_cell_assign: %llu alignments over more than SVG_CELL_MAX_GENES distinct genes", (unsigned long long)(uint32_t)tot[1]);
		return SVG_E_DEVICE;
	}
	if (r->ev[0]) {
		float ms = 0;
		if (with_barcode_event && hipEventElapsedTime(&ms, r->ev[0], r->ev[1]) == hipSuccess) ca->ms[1] += ms;
		if (hipEventElapsedTime(&ms, r->ev[4], r->ev[2]) == hipSuccess) ca->ms[0] += ms;
		if (hipEventElapsedTime(&ms, r->ev[2], r->ev[3]) == hipSuccess) ca->ms[2] += ms;
	}
	const uint64_t ng = tot[0];
	r->chunk_gene_base = r->n_genes;
	r->chunk_genes = ng;
	if (r->quiet) { r->n_hits += used; r->n_genes += ng; return 0; }
	if (r->n_genes + ng > r->cap_genes) {
		const uint64_t cap = (r->n_genes + ng) * 2;
		int32_t *g = (int32_t *)realloc(r->genes, 4 * cap);
		if (!g) { svg_set_error("out of host memory"); return SVG_E_NOMEM; }
		r->genes = g; r->cap_genes = cap;
	}
	if (ng && hipMemcpy(r->genes + r->n_genes, r->d_genes, 4 * ng, hipMemcpyDeviceToHost) != hipSuccess) {
		svg_set_error("svg_cell_assign: download failed");
		return SVG_E_DEVICE;
	}
	r->n_hits += used;
	r->n_genes += ng;
	return 0;
}

int cell_assign_chunk(CellAssignRun *r, uint64_t first_read, uint64_t k, const svg_cell_aln *d_recs, uint64_t used, const uint32_t *d_bases,
                      const uint32_t *d_xmask)
{
	svg_cellassign *ca = r->h->cas;
	if (used > r->cap_recs) { svg_set_error("svg_cell_assign: a chunk of %llu records", (unsigned long long)used); return SVG_E_DEVICE; }
	if (r->have_bc) {
		BarcodeParams bp;
		memset(&bp, 0, sizeof bp);
		bp.bt = ca->bt;
		bp.bases = (const uint32_t *)r->d_bases;
		bp.xmask = (const uint32_t *)r->d_xmask;
		bp.starts = r->d_starts ? (const uint64_t *)r->d_starts + first_read : NULL;
		bp.stride = r->stride;
		bp.base0 = first_read * r->stride;
		if (r->device_bc) { bp.bases = d_bases; bp.xmask = d_xmask; bp.starts = NULL; bp.stride = SVG_CELL_NAME_STRIDE; bp.base0 = 0; }
		bp.n = (uint32_t)k;
		bp.out = (int32_t *)r->d_bc;
		if (r->ev[0]) hipEventRecord(r->ev[0], r->st);
		hipLaunchKernelGGL(barcode_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, r->st, bp);
		if (r->ev[0]) hipEventRecord(r->ev[1], r->st);
		if (hipGetLastError() != hipSuccess ||
		    (!r->quiet && hipMemcpyAsync(r->bc + first_read, r->d_bc, 4 * k, hipMemcpyDeviceToHost, r->st) != hipSuccess)) {
			svg_set_error("svg_cell_assign_batch: HIP error %s", hipGetErrorString(hipGetLastError()));
			return SVG_E_DEVICE;
		}
	} else if (!r->quiet)
		for (uint64_t i = 0; i < k; i++) r->bc[first_read + i] = -1;
	r->chunk_gene_base = r->n_genes;
	r->chunk_genes = 0;
	int rc = run_records(r, d_recs, used, r->have_bc);
	if (rc) return rc;
	if (!used && r->have_bc) {
		if (hipStreamSynchronize(r->st) != hipSuccess) { svg_set_error("svg_cell_assign_batch: HIP error"); return SVG_E_DEVICE; }
		float ms = 0;
		if (r->ev[0] && hipEventElapsedTime(&ms, r->ev[0], r->ev[1]) == hipSuccess) ca->ms[1] += ms;
	}
	return 0;
}

void cell_assign_view(CellAssignRun *r, const svg_cell_hit **d_hits, const int32_t **d_genes, uint64_t *gene_base, uint64_t *n_genes,
                      const int32_t **d_bc)
{
	*d_hits = (const svg_cell_hit *)r->d_hits;
	*d_genes = (const int32_t *)r->d_genes;
	*gene_base = r->chunk_gene_base;
	*n_genes = r->chunk_genes;
	*d_bc = r->have_bc ? (const int32_t *)r->d_bc : NULL;
}

void cell_assign_end(CellAssignRun *r, svg_cell_hits *hits, int32_t **barcode_no)
{
	if (hits && barcode_no) {
		hits->n_records = r->n_hits;
		hits->n_genes = r->n_genes;
		hits->hits = r->hits;
		hits->genes = r->genes;
		*barcode_no = r->bc;
		r->hits = NULL; r->genes = NULL; r->bc = NULL;
	}
	run_free(r);
}

extern "C" void svg_cell_hits_free(svg_cell_hits *hits)
{
	if (!hits) return;
	free(hits->hits);
	free(hits->genes);
	memset(hits, 0, sizeof *hits);
}

extern "C" void svg_cell_assign_free(svg_cell_assigned *res)
{
	if (!res) return;
	svg_cell_align_free(&res->alns);
	svg_cell_hits_free(&res->hits);
	free(res->cell_barcode_no);
	memset(res, 0, sizeof *res);
}

static_assert(sizeof(svg_cell_hit) == 24 && sizeof(svg_cell_feature) == 20, "svg_cell_hit / svg_cell_feature layout");

extern "C" int svg_cell_assign_batch(svg_index *h, const svg_cell_align_params *p, const svg_packed_reads *reads,
                                     const svg_packed_reads *barcodes, svg_cell_assigned *res)
{
	if (!h || !p || !reads || !res) { svg_set_error("svg_cell_assign_batch: NULL argument"); return SVG_E_ARG; }
	memset(res, 0, sizeof *res);
	if (barcodes && barcodes->n_reads != reads->n_reads) {
		svg_set_error("svg_cell_assign_batch: %llu barcodes for %llu reads", (unsigned long long)barcodes->n_reads,
		              (unsigned long long)reads->n_reads);
		return SVG_E_ARG;
	}
	int rc = cell_align_run(h, p, reads, &res->alns, barcodes, &res->hits, &res->cell_barcode_no);
	if (rc) { svg_cell_assign_free(res); return rc; }
	return 0;
}

extern "C" int svg_cell_assign_records(svg_index *h, const svg_cell_aln *alns, uint64_t n, svg_cell_hits *hits)
{
	if (!h || !hits || (n && !alns)) { svg_set_error("svg_cell_assign_records: NULL argument"); return SVG_E_ARG; }
	memset(hits, 0, sizeof *hits);
	if (h->nblocks > 1) {
		svg_set_error("svg_cell_assign_records: an index of %d blocks (cellCounts takes a one-block index)", h->nblocks);
		return SVG_E_UNSUPPORTED;
	}
	if (!n) return 0;
	if (!cas_get(h)) return SVG_E_NOMEM;
	HIPCHK(hipSetDevice(h->device));
	hipStream_t st = h->stream;
	if (h->last_pending) HIPCHK(hipStreamWaitEvent(st, h->ev_last, 0));
	CellAssignRun *r = (CellAssignRun *)calloc(1, sizeof *r);
	if (!r) { svg_set_error("out of host memory"); return SVG_E_NOMEM; }
	r->h = h; r->st = st;
	const uint64_t CH = 1u << 17;
	const uint64_t m = n < CH ? n : CH;
	void *d_recs = NULL;
	int rc = run_buffers(r, m);
	if (!rc) rc = run_alloc(r, &d_recs, sizeof(svg_cell_aln) * m);
	for (uint64_t o = 0; o < n && !rc; o += m) {
		const uint64_t k = n - o < m ? n - o : m;
		if (hipMemcpyAsync(d_recs, alns + o, sizeof(svg_cell_aln) * k, hipMemcpyHostToDevice, st) != hipSuccess) {
			svg_set_error("svg_cell_assign_records: upload failed");
			rc = SVG_E_DEVICE;
			break;
		}
		rc = run_records(r, (const svg_cell_aln *)d_recs, k, 0);
	}
	hipFree(d_recs);
	if (!rc) {
		hits->n_records = r->n_hits; hits->n_genes = r->n_genes; hits->hits = r->hits; hits->genes = r->genes;
		r->hits = NULL; r->genes = NULL;
	}
	run_free(r);
	return rc;
}

extern "C" int svg_cell_assign_timing(svg_index *h, double ms[3])
{
	if (!h || !ms) { svg_set_error("svg_cell_assign_timing: NULL argument"); return SVG_E_ARG; }
	for (int i = 0; i < 3; i++) { ms[i] = h->cas ? h->cas->ms[i] : 0; if (h->cas) h->cas->ms[i] = 0; }
	return 0;
}
