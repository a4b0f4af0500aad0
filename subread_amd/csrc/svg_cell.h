// svg_cell.h -- what svg_cell.hip (the cellCounts vote) shares with svg_cell_align.hip (the step
// behind it): the kernels' parameter block and the launch of the probe and tally kernels.
#ifndef SVG_CELL_H
#define SVG_CELL_H
#include "svg_device.h"
#include "svg_keylookup.h"

#define C_SUB   20                                 // SCRNA_SUBREADS_HARD_LIMIT, cell-counts.c:29
#define C_SLOTS (SVG_CELL_ROWS * SVG_CELL_SPACE)   // 51
#define C_PRIME 66889u                             // VOTING_PRIME_NUMBER, cell-counts.c:2749
#define C_NEG   2048                               // IS_NEGATIVE_STRAND, subread.h:107
#define C_STACK 8                                  // ranges the sort's stack has room for (it holds at most 5)

struct CellParams {
	KeyTable kt;
	const uint32_t *vals;
	int gap, total_subreads, max_indel;
	// the chunk's reads: read r at base starts[r], or base0 + r * stride
	const uint32_t *bases, *xmask;
	const uint64_t *starts;
	uint64_t stride, base0;
	const uint16_t *lens;
	uint32_t n;
	uint2 *probes;             // [2 * C_SUB][n]
	svg_cell_head *heads;      // [n]
	svg_cell_slot *staging;    // [n][C_SLOTS]
	svg_cell_slot *compact;
	uint64_t slot_base;        // slots of the chunks before this one
	uint64_t *total;           // the chunk's slot count
};

__device__ __forceinline__ uint64_t cell_read_base(const CellParams &cp, uint32_t r)
{
	return cp.starts ? cp.starts[r] : cp.base0 + (uint64_t)r * cp.stride;
}

// cell_probe_kernel and cell_tally_kernel for one chunk on st: heads (first_slot unset) and the
// reads' 51 staging records each; mid (or NULL) is recorded between the two kernels
void cell_launch_vote(const CellParams &cp, int img, int n_cu, hipStream_t st, hipEvent_t mid = NULL);

// svg_cell_assign.hip behind svg_cell_align.hip's chunk loop (svg_cell_assign_batch): begin uploads
// the read barcodes (bc may be NULL) and takes the chunk buffers; chunk assigns the `used` records
// of the chunk that lie compacted at d_recs and the barcodes of its k reads from first_read on, and
// appends them to the run's host arrays; end hands the arrays over (hits and barcode_no NULL: frees
// them) and releases the run
struct CellAssignRun;
int  cell_assign_begin(svg_index *h, const svg_packed_reads *bc, uint64_t n, uint64_t chunk, int max_report, hipStream_t st,
                       CellAssignRun **out, bool quiet = false);
int  cell_assign_chunk(CellAssignRun *run, uint64_t first_read, uint64_t k, const svg_cell_aln *d_recs, uint64_t used);
void cell_assign_end(CellAssignRun *run, svg_cell_hits *hits, int32_t **barcode_no);
// the chunk's buffers in device memory after cell_assign_chunk: hits of its records, its compacted
// gene lists (n_genes numbers, the first being number gene_base of the run) and its reads' barcode
// numbers (NULL: no whitelist or no barcodes)
void cell_assign_view(CellAssignRun *run, const svg_cell_hit **d_hits, const int32_t **d_genes, uint64_t *gene_base, uint64_t *n_genes,
                      const int32_t **d_bc);
// svg_cell_count.hip behind the assignment (svg_cell_count_batch): begin uploads the reads' UMIs and
// sample numbers; chunk appends the chunk's observations to the counter
struct CellCountSink;
int  cell_count_begin(CellCountSink *sink, uint64_t n, hipStream_t st);
int  cell_count_chunk(CellCountSink *sink, uint64_t first_read, uint64_t k, const svg_cell_aln_head *d_heads, uint64_t rec_base,
                      const svg_cell_hit *d_hits, const int32_t *d_genes, uint64_t gene_base, uint64_t n_genes, const int32_t *d_bc,
                      hipStream_t st);
// svg_cell_align_batch's body; hits != NULL: with the assignment behind every chunk; sink != NULL:
// with the counter behind that; quiet: nothing per read is downloaded and res, hits and barcode_no
// stay empty
int  cell_align_run(svg_index *h, const svg_cell_align_params *p, const svg_packed_reads *reads, svg_cell_alns *res,
                    const svg_packed_reads *bc, svg_cell_hits *hits, int32_t **barcode_no, CellCountSink *sink = NULL, bool quiet = false);
#endif
