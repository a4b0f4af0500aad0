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
// device_bc: the barcodes are not uploaded; every chunk's lie in device memory (d_bases and d_xmask of
// cell_assign_chunk: read i of the chunk at base i * SVG_CELL_NAME_STRIDE)
int  cell_assign_begin(svg_index *h, const svg_packed_reads *bc, uint64_t n, uint64_t chunk, int max_report, hipStream_t st,
                       CellAssignRun **out, bool quiet = false, bool device_bc = false);
int  cell_assign_chunk(CellAssignRun *run, uint64_t first_read, uint64_t k, const svg_cell_aln *d_recs, uint64_t used,
                       const uint32_t *d_bases = NULL, const uint32_t *d_xmask = NULL);
// the whitelist's barcode length; 0: no whitelist
int  cell_assign_barcode_length(svg_index *h);
void cell_assign_end(CellAssignRun *run, svg_cell_hits *hits, int32_t **barcode_no);
// the chunk's buffers in device memory after cell_assign_chunk: hits of its records, its compacted
// gene lists (n_genes numbers, the first being number gene_base of the run) and its reads' barcode
// numbers (NULL: no whitelist or no barcodes)
void cell_assign_view(CellAssignRun *run, const svg_cell_hit **d_hits, const int32_t **d_genes, uint64_t *gene_base, uint64_t *n_genes,
                      const int32_t **d_bc);
// svg_cell_count.hip behind the assignment (svg_cell_count_batch): begin uploads the reads' UMIs and
// sample numbers; chunk appends the chunk's observations to the counter
// (svg_cell_count_names_batch: begin uploads the names instead, and parse runs the parse kernel over
// a chunk's names in front of cell_assign_chunk, whose barcodes are then the kernel's output)
struct CellCountSink;
const char *cell_count_who(CellCountSink *sink);
bool cell_count_has_names(CellCountSink *sink);
int  cell_count_begin(CellCountSink *sink, uint64_t n, uint64_t chunk, hipStream_t st);
int  cell_count_parse(CellCountSink *sink, uint64_t first_read, uint64_t k, const uint32_t **d_bc_bases, const uint32_t **d_bc_xmask);
int  cell_count_chunk(CellCountSink *sink, uint64_t first_read, uint64_t k, const svg_cell_aln_head *d_heads, uint64_t rec_base,
                      const svg_cell_hit *d_hits, const int32_t *d_genes, uint64_t gene_base, uint64_t n_genes, const int32_t *d_bc,
                      hipStream_t st);
// svg_cell_align_batch's body; hits != NULL: with the assignment behind every chunk; sink != NULL:
// with the counter behind that; quiet: nothing per read is downloaded and res, hits and barcode_no
// stay empty
int  cell_align_run(svg_index *h, const svg_cell_align_params *p, const svg_packed_reads *reads, svg_cell_alns *res,
                    const svg_packed_reads *bc, svg_cell_hits *hits, int32_t **barcode_no, CellCountSink *sink = NULL, bool quiet = false);
// svg_cell_names.hip: the names of a batch in device memory and one chunk's parse output.  begin
// uploads the text; chunk launches the parse kernel over k names (asynchronous on st); view gives the
// chunk's output arrays (k entries each; the packed words at SVG_CELL_NAME_STRIDE bases a name) and
// the run's count of refused names; time adds the last chunk's kernel time once st is idle
struct CellNamesRun;
struct CellNamesView {
	const int32_t *fields, *trimmed, *lane, *sample;
	const uint32_t *status, *bc_bases, *bc_xmask, *umi_bases, *umi_xmask;
	unsigned long long *refused;
};
int  cell_names_begin(svg_index *h, const char *who, const svg_reads *names, int mode, int bl, int ul, uint64_t n, uint64_t chunk, hipStream_t st,
                      CellNamesRun **out);
int  cell_names_chunk(CellNamesRun *run, uint64_t first_read, uint64_t k);
void cell_names_view(CellNamesRun *run, CellNamesView *v);
void cell_names_time(CellNamesRun *run);
void cell_names_end(CellNamesRun *run);
// svg_cell_set_samples' n_samples; 0: no sheet
int  cell_names_samples(svg_index *h);
#endif
