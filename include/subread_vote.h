/*
 * subread_vote.h -- C ABI of the MI355X seed-and-vote read-alignment hot path.
 *
 * Drop-in boundary for the voting step of Subread v2.0.6 (subread-align /
 * subjunc).  In the reference the step is the internal function
 *     int do_voting(global_context_t*, thread_context_t*)        core.c:3049
 * run once per pthread by run_in_thread(STEP_VOTING)             core.c:3366
 * It pulls reads from fetch_next_read_pair (core.c:1121), probes the sorted
 * hash table with gehash_go_X (sorted-hashtable.c:937), selects the top-K
 * candidates with process_voting_junction_PE_topK (core-junction.c:2199) and
 * writes up to multi_best mapping_result_t per read end into the bigtable
 * (core-bigtable.c:127) -- plus subjunc_result_t and the big-margin records in
 * subjunc mode.  svg_vote_batch() replaces that whole step for a batch of reads:
 * reads (ASCII, exactly what fetch_next_read_pair hands to do_voting before the
 * -S reversal) go in, the same bigtable records come out, byte for byte.
 *
 * Conventions (mirroring the reference): functions return 0 on success and a
 * negative SVG_E_* code on failure; the text of the last error of the calling
 * thread is available from svg_last_error().  The caller owns every host
 * buffer; the library owns device memory and streams.  One handle per GPU;
 * calls on one handle are serialised by the caller (one host thread).
 *
 * Nothing in this header depends on HIP or torch types.
 */
#ifndef SUBREAD_VOTE_H
#define SUBREAD_VOTE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVG_ABI_VERSION 2

/* reference constants (subread.h:73,88,216-217; core-junction.c:3569) */
#define SVG_MAX_READ_LENGTH       1210   /* MAX_READ_LENGTH == index padding */
/* the reference's reader keeps at most MAX_READ_LENGTH-1 bases of a read line
 * (read_line, input-files.c:277); longer reads are truncated the same way here */
#define SVG_READ_KEEP             (SVG_MAX_READ_LENGTH - 1)
#define SVG_MAX_INDEL_SECTIONS    7
#define SVG_VOTE_TABLE_SIZE       30     /* GENE_VOTE_TABLE_SIZE */
#define SVG_VOTE_SPACE            24     /* GENE_VOTE_SPACE */
#define SVG_BIG_MARGIN_WORDS      9      /* config.big_margin_record_size */
#define SVG_NEGATIVE_STRAND_FLAG  8      /* CORE_IS_NEGATIVE_STRAND in result_flags */

/* error codes */
#define SVG_OK               0
#define SVG_E_ARG          (-1)   /* bad argument / NULL pointer */
#define SVG_E_IO           (-2)   /* index file missing / unreadable */
#define SVG_E_FORMAT       (-3)   /* index file malformed */
#define SVG_E_UNSUPPORTED  (-4)   /* configuration outside the drop-in contract */
#define SVG_E_DEVICE       (-5)   /* HIP runtime failure */
#define SVG_E_NOMEM        (-6)

/* mapping_result_t, core.h:350-370 -- identical layout (68 bytes). */
typedef struct svg_mapping_result {
	uint32_t selected_position;
	int16_t  result_flags;
	int16_t  read_length;
	int16_t  selected_votes;
	int16_t  used_subreads_in_vote;
	uint8_t  noninformative_subreads_in_vote;
	int8_t   indels_in_confident_coverage;
	int8_t   is_fully_covered;
	uint8_t  _pad0;
	int16_t  selected_indel_record[SVG_MAX_INDEL_SECTIONS * 3 + 1];
	uint16_t confident_coverage_start;
	uint16_t confident_coverage_end;
	int16_t  subread_quality;
	uint16_t _pad1;
} svg_mapping_result;

/* subjunc_result_t, core.h:397-410 -- identical layout (16 bytes). */
typedef struct svg_subjunc_result {
	int16_t  split_point;
	int16_t  minor_votes;
	int8_t   double_indel_offset;
	int8_t   indel_at_junction;
	int8_t   small_side_increasing_coordinate;
	int8_t   large_side_increasing_coordinate;
	uint32_t minor_position;
	uint16_t minor_coverage_start;
	uint16_t minor_coverage_end;
} svg_subjunc_result;

/*
 * Voting parameters: the subset of configuration_t (core.h:128-253) the vote
 * path reads.  svg_params_default() fills them exactly as the reference does:
 * init_global_context (core-indel.c:4399-4538), then parse_opts_aligner /
 * parse_opts_subjunc (core-interface-aligner.c:256, core-interface-subjunc.c:255),
 * then the runtime overrides of load_global_context (core.c:4075-4094).
 */
typedef struct svg_params {
	int32_t total_subreads;               /* -n                      (10 align, 14 subjunc) */
	int32_t min_votes_first;              /* -m minimum_subread_for_first_read  (3 / 1)   */
	int32_t min_votes_second;             /* -p minimum_subread_for_second_read (1)       */
	int32_t max_indel_length;             /* -I  (voting uses min(16, I))        (5)      */
	int32_t multi_best;                   /* multi_best_reads                    (3)      */
	int32_t top_scores;                   /*                                     (3)      */
	int32_t max_vote_simples;             /* 3 SE / 64 PE, max'ed with -B                 */
	int32_t max_vote_combinations;        /* 3, max'ed with -B                            */
	int32_t max_vote_number_cutoff;       /*                                     (2)      */
	int32_t min_pair_distance;            /* -d                                  (50)     */
	int32_t max_pair_distance;            /* -D                                  (600)    */
	int32_t reverse_r1;                   /* is_first_read_reversed  (-S)        (0)      */
	int32_t reverse_r2;                   /* is_second_read_reversed (-S)        (1)      */
	int32_t do_breakpoint_detection;      /* subjunc                             (0 / 1)  */
	int32_t do_big_margin_filtering_for_junctions; /* subjunc                    (0 / 1)  */
	int32_t big_margin_record_size;       /*                                     (9)      */
	int32_t maximum_intron_length;        /*                                     (500000) */
	int32_t prefer_donor_receptor_junctions; /*                                  (1)      */
	int32_t check_donor_at_junctions;     /*                                     (1)      */
	int32_t max_insertion_at_junctions;   /*                                     (0)      */
	int32_t more_accurate_fusions;        /*                                     (1)      */
} svg_params;

#define SVG_PROGRAM_ALIGN   0   /* subread-align */
#define SVG_PROGRAM_SUBJUNC 1   /* subjunc */
void svg_params_default(svg_params *p, int program, int paired_end);

/*
 * A batch of reads as ASCII text.  Read i is seq[offsets[i] .. offsets[i]+lens[i]).
 * Reads are given as the FASTQ holds them (after trimming); the -S reversal
 * (reverse_r1 / reverse_r2) is applied inside the library exactly like
 * fetch_next_read_pair (core.c:1186-1198).  For paired-end input r1 and r2 hold
 * the same number of reads.  Read numbering in a batch = array order.
 */
typedef struct svg_reads {
	const char     *seq;
	const uint64_t *offsets;
	const uint16_t *lens;
	uint64_t        n_reads;
} svg_reads;

/*
 * The same reads 2-bit packed: ~4x fewer bytes to move than ASCII.
 *   bases : base2int codes (subread.h:238: A=0 G=1 C=2 T=3; any other character 2 if it
 *           sorts below 'G', else 3), 16 per word; base k of the stream in bits
 *           31-2(k%16) .. 30-2(k%16) of word k/16, so 16 bases starting at a word boundary
 *           read as genekey2int's key (input-files.c:1232).
 *   xmask : NULL when every base is A/C/G/T/U; else 1 bit per base (bit 31-(k%32) of word
 *           k/32) set for any other character (N, '.', lowercase, IUPAC ...).  Those all
 *           complement to 'N' in reverse_read (input-files.c:1111) and never match the
 *           genome there; 'U' behaves as 'T' everywhere and packs as T.  (A read holds no
 *           NUL byte -- it would end the reference's C string.)
 *   starts: base index of read i in the stream; NULL = i * stride.
 * Read i = bases starts[i] .. starts[i]+lens[i]-1.  svg_pack_reads() builds this form.
 */
typedef struct svg_packed_reads {
	const uint32_t *bases;
	const uint32_t *xmask;
	const uint64_t *starts;
	uint64_t        stride;
	const uint16_t *lens;
	uint64_t        n_reads;
} svg_packed_reads;

/* Pack ASCII reads: with starts != NULL the reads go back to back (starts[i] filled in,
 * bases sized ceil(sum(lens)/16) words, xmask ceil(sum(lens)/32)); with starts == NULL read
 * i goes to base i*stride (every lens[i] <= stride; n*stride bases).  Returns the number of
 * exception bases (0: the caller may pass xmask = NULL to the vote) or a negative SVG_E_*. */
int64_t svg_pack_reads(const svg_reads *in, uint64_t stride, uint32_t *bases, uint32_t *xmask, uint64_t *starts,
                       int threads);

/* opaque index handle: owns the HBM copy of every <prefix>.NN.b.tab / .array block and .reads */
typedef struct svg_index svg_index;

typedef struct svg_index_info {
	uint64_t items;              /* hashed 16-mers in the .tab                 */
	uint32_t buckets;            /* buckets_number                             */
	int32_t  index_gap;          /* 1 (-F full index) or 3 (gapped)            */
	int32_t  padding;            /* 1210                                       */
	uint32_t array_length;       /* .array length (bases incl. padding)        */
	uint32_t n_chromosomes;
	uint64_t device_bytes;       /* HBM held by the handle                     */
	int32_t  device;             /* HIP device ordinal                         */
	uint32_t array_values_bytes; /* bytes of the packed .array image           */
	int32_t  n_blocks;           /* index blocks (<prefix>.NN.b.*); the fields above
	                                but device_bytes describe block 00           */
} svg_index_info;

/* Load a base-space index as written by subread-buildindex -- "<prefix>.NN.b.tab" and
 * "<prefix>.NN.b.array" for every block NN = 00, 01, ... and "<prefix>.reads" -- into HBM of
 * `device`.  All blocks stay resident; a vote runs them in order, each later block merging
 * with the records the earlier ones left (read_chunk_circles, core.c:3567-3613), so a
 * multi-block index gives the reference's records for the same reads. */
int  svg_index_open(const char *prefix, int device, svg_index **out);
/* The same for n devices at once (out[k] on devices[k]; a device may repeat: several replicas on
 * one GPU): the files are read, walked and staged once and every staged run is copied to every
 * replica -- an 8-GPU node loads the index once instead of eight times.  All or nothing: on an
 * error no handle is left open. */
int  svg_index_open_devices(const char *prefix, const int *devices, int n, svg_index **out);
void svg_index_close(svg_index *idx);
int  svg_index_get_info(const svg_index *idx, svg_index_info *out);

/*
 * Build an index straight into HBM, from a FASTA file or from in-memory contigs, with the block
 * structure subread-buildindex gives it for `memory_mb` (-M): one block if force_one_block (-B)
 * is set or no block ever closes, else as many as build_gene_index splits off (at most 64: beyond
 * that SVG_E_UNSUPPORTED).  Every block stays resident, as after svg_index_open;
 * svg_index_get_info().n_blocks reports their number.  The items are those of svg_build_index /
 * subread-buildindex; when save_prefix is not NULL the reference-format files of every block
 * (and .reads / .files / .log) are also written there, and blocks a previous build left behind
 * are removed.
 */
int  svg_index_build(const char *fasta, int gap, int memory_mb, int force_one_block,
                     int repeat_threshold, int device, const char *save_prefix, svg_index **out);
int  svg_index_build_mem(const char *const *names, const char *const *seqs, const uint64_t *lens,
                         uint32_t n_contigs, int gap, int memory_mb, int force_one_block,
                         int repeat_threshold, int device, const char *save_prefix, svg_index **out);
/* Copy block 00 of the index back to host arrays (any pointer may be NULL): bstart[buckets+1],
 * keys[items], vals[items], values[array_values_bytes], chr_end[n_chromosomes]. */
int  svg_index_export(const svg_index *idx, uint32_t *bstart, int16_t *keys, uint32_t *vals,
                      uint8_t *values, uint32_t *chr_end);

/*
 * Vote a batch.  Host buffers in, host buffers out (synchronous).
 *   out   : n_reads * ends * multi_best records, index ((read*ends)+end)*multi_best+best
 *   jout  : same shape, subjunc_result_t; required iff do_breakpoint_detection
 *   big_margin : n_reads * ends * SVG_BIG_MARGIN_WORDS; required iff
 *           do_big_margin_filtering_for_junctions (reference bigtable
 *           big_margin_data, core.h:453)
 * r2 == NULL means single-end.  Output buffers are fully overwritten (the
 * reference zeroes the bigtable per chunk, core-bigtable.c:84-125).
 */
int svg_vote_batch(svg_index *idx, const svg_params *p,
                   const svg_reads *r1, const svg_reads *r2,
                   svg_mapping_result *out, svg_subjunc_result *jout,
                   uint16_t *big_margin);
/* The same from 2-bit packed reads (host buffers).  Both host entry points run a sub-batch
 * pipeline: upload of sub-batch i+1, vote of i (probe + lane kernels) beside the wave kernel and
 * compaction of i-1, download of i-2 (only the non-zero records, compacted on the GPU) and
 * expansion of i-3 into `out` by worker threads overlap.  Workers: svg_host_threads().  Pinned caller buffers copy fastest. */
int svg_vote_batch_packed(svg_index *idx, const svg_params *p,
                          const svg_packed_reads *r1, const svg_packed_reads *r2,
                          svg_mapping_result *out, svg_subjunc_result *jout,
                          uint16_t *big_margin);

/*
 * Same computation on device-resident buffers, asynchronous on `hip_stream`
 * (a hipStream_t passed as void*, NULL = the handle's own stream).  Every
 * pointer in r1/r2 and the outputs is a device pointer.
 */
int svg_vote_batch_device(svg_index *idx, const svg_params *p,
                          const svg_reads *r1, const svg_reads *r2,
                          svg_mapping_result *out, svg_subjunc_result *jout,
                          uint16_t *big_margin, void *hip_stream);
/* Packed reads in device memory (unpacked on the GPU into a buffer of the handle, sized by
 * svg_set_max_read_length's bound), asynchronous on `hip_stream`. */
int svg_vote_batch_packed_device(svg_index *idx, const svg_params *p,
                                 const svg_packed_reads *r1, const svg_packed_reads *r2,
                                 svg_mapping_result *out, svg_subjunc_result *jout,
                                 uint16_t *big_margin, void *hip_stream);

/*
 * Equal-key runs of arbitrary subread keys in one index block: cellCounts' hit-list lookup
 * (prefill_votes, cell-counts.c:432-491) on the GPU.  For key i: bucket b = key % buckets,
 * binary search of (short)(key / buckets) in the bucket's keys, then prefill_votes' step-down
 * widening, exactly.  first[i] = bucket-local index of the run's first item (the reference's
 * start_location_in_index = bucket->item_values + first[i]), count[i] = run length (its
 * votes[i]; 0 = absent, first[i] = 0).  svg_probe_keys takes host buffers (synchronous);
 * svg_probe_keys_device device buffers, asynchronous on hip_stream (NULL: the handle's).
 */
int svg_probe_keys(svg_index *idx, int block, const uint32_t *keys, uint64_t n,
                   uint32_t *first, uint32_t *count);
int svg_probe_keys_device(svg_index *idx, int block, const uint32_t *keys, uint64_t n,
                          uint32_t *first, uint32_t *count, void *hip_stream);

/*
 * cellCounts' voting step for a batch of reads (cellCounts_do_voting, cell-counts.c:3051-3131, up
 * to the call of cellCounts_select_and_write_alignments).  Per read the reference looks up every
 * subread of both strands (prefill_votes, :3085-3101: one key per subread at offset
 * (step * k) >> 16, no gap-slot loop) and then tallies the hit lists into a private 17-row x
 * 3-slot table shared by both strands (cellCounts_process_copy_ptrs_to_votes, :2786-2881:
 * subreads in ascending order of hit count under quick_sort_run's permutation, core.c:4694-4714;
 * hits of a run visited at (sum += 66889) % run; the indel recorder keyed by distance).  Nothing
 * outside the read is touched, so the step is a function of the read, the one-block index,
 * total_subreads and max_indel_length: svg_cell_vote_batch runs it on the GPU and returns the
 * tables (host buffers, synchronous; the result arrays are owned by the library until
 * svg_cell_vote_free).
 *   total_subreads    --subreadsPerRead, 7..20 (the reference's clamp, :547); default 10
 *   max_indel_length  5: cellCounts' option parsing never changes it (:521)
 * Other values are SVG_E_ARG, as is a read of more than SVG_CELL_MAX_READ_LENGTH bases; an index
 * of several blocks is SVG_E_UNSUPPORTED (cellCounts refuses it, :641-644).  A read under 16
 * bases gets a zero head and no slots (:3077).
 * Limit: the tables are the reference's for indexes whose hit lists (equal-key runs) hold at most
 * 32,000 items.  Past that the reference's int sum of 66889 * run overflows and it reads before
 * the list; here the sum is unsigned and stays inside the list.  subread-buildindex's default
 * repeat threshold (-f 100) keeps every list under 100 items.
 * A caller fills a gene_sc_vote_t (cell-counts.c:37-64) field by field: max_vote and items[]
 * from the head; pos, masks, votes, toli, coverage_start / _end and indel_recorder[0..toli) of
 * slot [row][k] from slots[first_slot + items[0] + .. + items[row-1] + k].  Fields the tally never
 * writes (quality, cursors, the max_* fields but max_vote, recorder entries past toli) are not
 * part of the result.
 */
#define SVG_CELL_ROWS             17    /* GENE_SCRNA_VOTE_TABLE_SIZE */
#define SVG_CELL_SPACE            3     /* GENE_SCRNA_VOTE_SPACE */
#define SVG_CELL_RECORDER         21    /* MAX_INDEL_TOLERANCE * 3 */
#define SVG_CELL_MAX_READ_LENGTH  160   /* MAX_SCRNA_READ_LENGTH */

typedef struct svg_cell_params {
	int32_t total_subreads;
	int32_t max_indel_length;
} svg_cell_params;

typedef struct svg_cell_head {
	uint64_t first_slot;              /* the read's first record in slots */
	uint16_t n_slots;                 /* sum of items[] */
	int16_t  max_vote;
	int16_t  applied_subreads;        /* per strand; 0 for a read under 16 bases */
	uint8_t  items[SVG_CELL_ROWS];
	uint8_t  _pad;
} svg_cell_head;                      /* 32 bytes */

typedef struct svg_cell_slot {
	uint32_t pos;
	int16_t  mask;                    /* 0, or IS_NEGATIVE_STRAND (2048) */
	int16_t  votes;
	int16_t  coverage_start, coverage_end;
	uint8_t  toli;
	uint8_t  _pad;
	int16_t  indel_recorder[SVG_CELL_RECORDER];   /* zero from toli on */
} svg_cell_slot;                      /* 56 bytes */

typedef struct svg_cell_votes {
	uint64_t n_reads, n_slots;
	svg_cell_head *heads;             /* one per read, batch order */
	svg_cell_slot *slots;             /* read by read, each read's in row-major slot order */
} svg_cell_votes;

int  svg_cell_vote_batch(svg_index *idx, const svg_cell_params *p, const svg_packed_reads *reads,
                         svg_cell_votes *res);
void svg_cell_vote_free(svg_cell_votes *res);

/*
 * cellCounts' voting step and, behind it on the GPU, everything that
 * cellCounts_select_and_write_alignments does (cell-counts.c:2648-2719) up to, but not including,
 * its calls of cellCounts_write_read_in_batch_bin: the choice of at most max_voting_simples slots
 * of the table (:2654-2686, cellCounts_update_top_three :2296-2310), cellCounts_explain_one_read
 * for each (:2520-2627: cellCounts_indel_recorder_copy :2352-2424, cellCounts_find_soft_clipping
 * :326-396, cellCounts_meet_in_the_middle :2462-2506, cellCounts_matchBin_chro :2426-2458,
 * find_subread_end input-files.c:1371-1377, cellCounts_reduce_Cigar :238-265,
 * cellCounts_calculate_pos_weight :1535-1571, cellCounts_test_score :2508-2511), the quick_sort
 * of the scores (:2691-2698; core.c:4690-4714, unstable: ties come out in its order) and the
 * choice of the records to write (:2700-2716).  The vote tables stay on the device.
 *
 * Per read (batch order) one svg_cell_aln_head: reporting_multi_alignment_no after its min with
 * max_reported_alignments_per_read, the number of its records and the index of the first; no
 * records = the reference writes the read as unmapped.  Per call of the writer with a
 * reporting_index >= 0, in the order of the calls, one svg_cell_aln: reporting_positions (0-based
 * linear, before the writer's + 1 and locate_gene_position), reporting_flags (0 or 16),
 * reporting_mapq, reporting_editing_distance, reporting_scores and the reduced CIGAR as text.
 * locate_gene_position ("no chromosome: unmapped"), the feature lookup and the writers stay with
 * the caller.
 *
 * The CIGAR field.  A record is written for a score > 0 only, i.e. rebuilt_rlen == read_len <= 160:
 * the counts of the text's M, S and I pieces are positive and sum to at most 160.  The table slot
 * has at most 7 sections (toli <= 21), so explain_one_read appends at most 6 pieces
 * "%dM%dM%d%c%dM" between the head "%dS" and the tail "%dM" "%dS".  Of a piece's numbers only
 * the second and fourth can be negative ('-' is an operation of count 1 to reduce_Cigar: "1-"),
 * as can the tail's M.  After the merge of equal neighbours that leaves at most 22 M/S/I pieces
 * (S, 3 M + I, 5 x (2 M + I), M, S), 13 "1-" and 6 D of one digit (|indel| < 5; merged ones are
 * fewer pieces).  22 positive counts that sum to <= 160 have at most 37 digits (at most 15 of
 * them reach 10), so the text has at most 22 + 37 + 26 + 12 = 97 characters: SVG_CELL_CIGAR = 108
 * holds it with its NUL and rounds the record to 128 bytes.
 *
 * Parameters (svg_cell_align_params_default: the defaults of cell-counts.c:517-529; ranges: the
 * clamps of :538-569; outside them SVG_E_ARG):
 *   total_subreads                         7..20, default 10
 *   max_indel_length                       5
 *   min_votes_per_mapped_read              1..64, default 3
 *   max_differential_from_top_vote_number  1..30, default 2
 *   max_mismatching_bases_in_reads         0..100, default 3
 *   min_mapped_length_for_mapped_read      -1..160, default 40
 *   max_reported_alignments_per_read       1..30, default 1
 * max_voting_simples is max(3, max_reported_alignments_per_read) (:518, :604) and
 * max_distinct_top_vote_numbers 3 (:522).  A multi-block index is SVG_E_UNSUPPORTED.
 *
 * The exon weight (:1535-1571) is read from two bit planes, exon bases and exon bases with 100
 * bases of flank, that svg_cell_set_exons fills from inclusive linear intervals as :938-959 fill
 * exonic_region_bitmap: an interval with an end above 0xffffff00 sets nothing (:941), and the
 * flank loop starts at the unsigned start - 100, so an exon that starts below 100 gets no flank
 * bits at all.  The planes cover the linear positions below the end of the .array image plus
 * SVG_CELL_EXON_TAIL; a bit beyond them is not set and reads as 0.  A later call replaces the
 * list; n = 0 clears it.  With no exons set every weight is 10.
 *
 * Outside the reference's contract, and memory-safe here:
 *   - cellCounts_get_index_int has no bounds check.  Where a candidate's soft-clip scan or
 *     meet-in-the-middle asks for a genome base outside the .array image the reference's answer
 *     is undefined; this library reads such a base as code 0.  (matchBin_chro checks, and returns
 *     0, in the reference too.)
 *   - a read with one subread per strand (16 .. 16 + gap bases): find_subread_end divides by zero
 *     in the reference as soon as a slot is explained; here such a read has a zero head.
 *   - a slot whose recorder copies to 7 sections makes indel_recorder_copy write one element past
 *     its array (:2402); here the write is dropped.
 * A candidate with a score > 0 whose text does not fit SVG_CELL_CIGAR (the bound above says there
 * is none) is counted on the device and fails the call with SVG_E_DEVICE.
 * With svg_set_timing on, svg_cell_align_timing returns, and resets, the milliseconds (HIP events
 * around each launch) summed per kernel since the last call: probe, tally, select, explain, emit,
 * scan + compact.
 */
#define SVG_CELL_CIGAR       108
#define SVG_CELL_EXON_TAIL   512
#define SVG_CELL_MAX_REPORT  30     /* SCRNA_HIGHEST_REPORTED_ALIGNMENTS */

typedef struct svg_cell_align_params {
	int32_t total_subreads;
	int32_t max_indel_length;
	int32_t min_votes_per_mapped_read;
	int32_t max_differential_from_top_vote_number;
	int32_t max_mismatching_bases_in_reads;
	int32_t min_mapped_length_for_mapped_read;
	int32_t max_reported_alignments_per_read;
} svg_cell_align_params;

typedef struct svg_cell_aln_head {
	uint64_t first_record;            /* the read's first record in alns (0 where it has none) */
	uint16_t n_records;
	uint16_t multi_alignment_no;      /* reporting_multi_alignment_no */
	uint32_t _pad;
} svg_cell_aln_head;                  /* 16 bytes */

typedef struct svg_cell_aln {
	int64_t  score;                   /* reporting_scores */
	uint32_t position;                /* reporting_positions */
	int16_t  flags;                   /* reporting_flags: 0, or 16 */
	int16_t  mapq;                    /* reporting_mapq */
	int32_t  editing_distance;        /* reporting_editing_distance */
	char     cigar[SVG_CELL_CIGAR];   /* reporting_cigars, NUL-terminated, zero to the end */
} svg_cell_aln;                       /* 128 bytes */

typedef struct svg_cell_alns {
	uint64_t n_reads, n_records;
	svg_cell_aln_head *heads;         /* one per read, batch order */
	svg_cell_aln *alns;               /* read by read, in the order of the writer's calls */
} svg_cell_alns;

void svg_cell_align_params_default(svg_cell_align_params *p);
int  svg_cell_set_exons(svg_index *idx, const uint32_t *starts, const uint32_t *stops, uint64_t n);
int  svg_cell_align_batch(svg_index *idx, const svg_cell_align_params *p, const svg_packed_reads *reads,
                          svg_cell_alns *res);
void svg_cell_align_free(svg_cell_alns *res);
int  svg_cell_align_timing(svg_index *idx, double ms[6]);

/*
 * The rest of what cellCounts computes per read before it only writes files: for every call of
 * cellCounts_write_read_in_batch_bin that svg_cell_align_batch records, the gene assignment of
 * the alignment (cell-counts.c:2061-2088, cellCounts_find_hits_for_mapped_section :1575-1654,
 * cellCounts_summarize_entrez_hits :2039-2059), the multi-overlap rule (:1982) and, per read, the
 * cell barcode (cellCounts_get_cellbarcode_no :1701-1768).  svg_cell_assign_batch returns what
 * svg_cell_align_batch returns, in the same layout (res->alns), and beside it
 *   hits[k]  for alns.alns[k]: the contig (index into the .reads table), or -1 where the reference
 *            turns the call into an unmapped one (locate_gene_position(position + 1) leaves
 *            chro_name NULL, gene-algorithms.c:441-511 with rl = 0: a position inside a contig's
 *            leading padding, past the last base that lies 15 bases short of the next padding, or
 *            beyond the last contig; chro_pos and nhits are then 0, as in the call of :2087);
 *            chro_pos as cellCounts_vote_and_add_count gets it (after get_soft_clipping_length is
 *            added, core.c:1232: the count of a head S only); nhits after the summary and after
 *            the rule of :1982; first_gene, where its nhits gene numbers start in genes;
 *   genes    the gene numbers in the reference's hits_indices order (first seen first);
 *   cell_barcode_no  per read, the whitelist number or -1.
 * svg_cell_assign_records runs the same assignment over records the caller holds in host memory.
 *
 * The walk follows the reference as written.  Every M section of the CIGAR text is looked up as
 * [chro_pos, chro_pos + length], both ends inclusive: the cursor of :2073-2083 never advances
 * (add_curs is computed and not added), and neither does it here.  A section starts at the
 * reverse-table bucket min(begin / 131072, chro_possible_length / 131072), skips unset buckets up
 * to min((1 + end) / 131072, chro_possible_length / 131072 + 1) (:1602-1609), walks the blocks
 * from there to the contig's last (break on block_min_start > end, continue on block_max_end <
 * begin) and the items of a block (stop >= begin, then break on start > end), and takes an item
 * whose strand equals the record's flag 16.
 *
 * svg_cell_set_annotation takes the features in annotation-file order: the contig as an index
 * into the handle's .reads table (the caller resolves names, the chr-prefix fallbacks of :897-906
 * and :1581-1596 included, and leaves out a feature on no contig of the index), start and end
 * 1-based inclusive as the annotation gives them, the strand (1 = '-') and the caller's gene
 * number (the reference numbers genes by first appearance, :1163).  On the host it builds what
 * cellCounts_sort_feature_info builds (:1099-1251): each contig's features by start under the
 * reference's merge_sort (core.c:4736-4753: selection sort of runs of at most 11, and a merge
 * that on equal starts takes the second run's item first, so ties are not in file order), the
 * blocks with the sqrt-sized bins of :1180, the reverse tables, chro_possible_length (:1275: the
 * difference of the .reads offsets, padding included; :920: raised to end + 1).  It also fills the
 * two exon planes of svg_cell_set_exons from linear_gene_position of start and end (:939-940)
 * through the same code.  A later call replaces everything, n = 0 clears the annotation and the
 * planes.  allow_multi_overlap is allow_multi_overlapping_reads.  SVG_E_ARG: a contig index out
 * of range, start > end (the reference's assert of :984), a strand above 1, and a feature whose
 * (end + 1) / 131072 + 2 exceeds the (length + 1 Mbase) / 131072 + 2 buckets that the reference
 * allocates for its contig's reverse table (:1277-1278) and writes without a check (:935, :1181).
 *
 * svg_cell_set_barcodes takes the whitelist as n strings of `length` characters: 2..16, A/C/G/T
 * only, distinct; anything else is SVG_E_ARG with the reason in svg_last_error.  n = 0 clears it.
 * The device image is the barcodes as 2-bit codes in whitelist order and the two half-key lists of
 * cellCounts_make_barcode_HT_table (:272-304; F: even positions, S: odd ones, length / 2
 * characters each) as direct-indexed CSR rows of 4 ^ (length / 2) keys, each row in ascending
 * whitelist order.  There is no third table for the exact probe: a barcode equal to a whitelist
 * entry has its F key, so the F row answers it.  The reference's order holds: the exact entry
 * wins wherever it stands; else the first entry of the F row, then of the S row, whose
 * hamming_dist_ATGC_max2 (input-blc.c:1109-1120) is exactly 1 (an entry of both rows was tested
 * in the F row already, so skipping it in the S row, as :1738-1745 do, changes nothing).
 * Read barcodes come as a second svg_packed_reads of the same count, `length` bases each.  An
 * exception bit stands for 'N': is_ATGC (input-blc.c:1054) accepts N, so the comparison goes on
 * past it and the N counts as one mismatch; a half key with an N matches no row.  Any other
 * character, at which hamming_dist_ATGC_max2 would stop, is outside this contract.
 * barcodes = NULL or no whitelist: cell_barcode_no -1 for every read.  No annotation: nhits 0
 * everywhere, contig and chro_pos still filled.
 *
 * Bound: a record holds at most SVG_CELL_MAX_GENES distinct genes.  With allow_multi_overlap 0
 * the bound cannot be met (two genes already make nhits 0); with it set, an alignment over more
 * distinct genes is counted on the device and fails the call with SVG_E_DEVICE, never truncated.
 * Outside the reference's contract: an alignment over more than MAX_HIT_NUMBER (10^6) features
 * stops the reference's section scan with an error message; here the scan goes on.
 * svg_cell_assign_timing (under svg_set_timing) returns and resets the summed milliseconds of
 * the assign kernel, the barcode kernel and the gene scan + compact.
 */
#define SVG_CELL_MAX_GENES 16

typedef struct svg_cell_feature {
	uint32_t contig;                  /* index into the .reads table */
	uint32_t start, end;              /* 1-based, inclusive */
	int32_t  gene;
	uint8_t  is_negative_strand;
	uint8_t  _pad[3];
} svg_cell_feature;                   /* 20 bytes */

typedef struct svg_cell_hit {
	int32_t  contig;                  /* -1: written as unmapped */
	int32_t  chro_pos;
	uint32_t nhits;
	uint32_t _pad;
	uint64_t first_gene;              /* genes[first_gene .. first_gene + nhits) (0 where nhits is 0) */
} svg_cell_hit;                       /* 24 bytes */

typedef struct svg_cell_hits {
	uint64_t n_records, n_genes;
	svg_cell_hit *hits;               /* one per svg_cell_aln */
	int32_t *genes;
} svg_cell_hits;

typedef struct svg_cell_assigned {
	svg_cell_alns alns;               /* as svg_cell_align_batch returns it */
	svg_cell_hits hits;
	int32_t *cell_barcode_no;         /* one per read */
} svg_cell_assigned;

int  svg_cell_set_annotation(svg_index *idx, const svg_cell_feature *features, uint64_t n, int allow_multi_overlap);
int  svg_cell_set_barcodes(svg_index *idx, const char *const *barcodes, uint64_t n, int length);
int  svg_cell_assign_batch(svg_index *idx, const svg_cell_align_params *p, const svg_packed_reads *reads,
                           const svg_packed_reads *barcodes, svg_cell_assigned *res);
void svg_cell_assign_free(svg_cell_assigned *res);
int  svg_cell_assign_records(svg_index *idx, const svg_cell_aln *alns, uint64_t n, svg_cell_hits *hits);
void svg_cell_hits_free(svg_cell_hits *hits);
int  svg_cell_assign_timing(svg_index *idx, double ms[3]);

/*
 * cellCounts' UMI stage: what cellCounts_do_one_batch (cell-counts.c:3951-4126) computes between
 * reading a batch file and rewriting it, as a counter object in device memory beside a handle.
 *
 * An observation is one (sample, cell, gene, UMI): the reference makes one per (written record,
 * gene of its list) with ADD_key_struct (:3945-3949, :4011-4026).  svg_cell_counter_finish runs
 *   1. the support count: the number of observations of every distinct (sample, cell, gene, UMI)
 *      (the string table of :3991 and cellCounts_do_one_batch_tab_to_struct_list, :3756-3775);
 *   2. step 1 (:4057-4058): per sample the entries by (cell, gene, support descending, UMI by
 *      memcmp) (the comparator of :3725-3754, a total order on distinct entries), then within each
 *      (cell, gene) section, in that order, an entry is merged into the first accepted entry at
 *      Hamming distance < 2 (cellCounts_hamming_max2_fixlen, :3511), whose support grows by the
 *      entry's; otherwise it is accepted (cellCounts_do_one_batch_UMI_merge_one_cell, :3552-3641).
 *      In a section of at most 30 entries "first" is the acceptance order (:3598-3620).  In a
 *      larger one (sec_end - sec_start > 30, :3555) it is the acceptance order among the acceptors
 *      whose first L/2 characters equal the entry's, and only if none of those is near, among the
 *      acceptors whose characters L/2 .. 2*(L/2)-1 equal the entry's (:3566-3597); for odd L the
 *      last character is in neither key.  The two rules pick different acceptors;
 *   3. step 2 (:4062-4064): the survivors by (cell, UMI, support descending, gene); a (cell, UMI)
 *      section of one entry counts 1 for its (cell, gene) (:3672); in a larger one the first counts
 *      1 only if its support is strictly greater than the second's, else removed_umis grows by one
 *      (:3532-3538); every other entry of the section is dropped;
 *   4. the (cell, gene) -> number of UMIs table (ADD_count_hash, :3520, written at :4068-4069).
 * Read as written and kept: the keys put into filtered_CGU_table are formatted after cellbc was
 * set to -1 (:3581-3587, :3540-3546), so the lookup of :4095-4102 never finds them for a real cell
 * and the replacement UMI is dead in the reference; this interface reports the acceptor's UMI per
 * entry and rewrites no read bin.
 *
 * Key fields (an observation is two 64-bit words): sample 1..255 (8 bits, at most n_samples), cell
 * 0..2^24-1 (24 bits: a whitelist of 2^23 barcodes fits), gene 0..2^31-1 (32 bits), the UMI as 3
 * bits a base with A < C < G < N < T (42 bits for SVG_CELL_MAX_UMI bases, so that an unsigned
 * compare of codes is memcmp of the text); a support is a uint32_t, and a counter holds fewer than
 * 2^31 observations (SVG_E_UNSUPPORTED beyond).  svg_cell_counter_add refuses a value outside its
 * field, and a UMI character other than A/C/G/T/N, with SVG_E_ARG and appends nothing;
 * svg_cell_count_batch counts such values on the device and svg_cell_counter_finish then fails
 * with SVG_E_ARG, on every call until svg_cell_counter_reset (the counter cannot tell which of its
 * observations the refused ones would have been).  Both paths check the fields before they drop
 * anything: sample 0 with a cell of 2^24 is refused, not dropped.  Never truncated.  An observation whose sample is <= 0, or whose cell is < 0
 * (both merge steps skip cell -1, :3658), is dropped and tallied (dropped_no_sample first,
 * dropped_no_cell second).
 *
 * svg_cell_count_batch runs svg_cell_assign_batch's chunk loop and, while a chunk's hits, gene lists
 * and barcode numbers are in device memory, appends one observation per (record, gene) of every
 * read: a record with contig -1 or nhits 0 gives none.  umis: `umi_length` bases per read, the
 * exception bit meaning N; sample_no: one int32 per read, cellCounts_get_sample_id's 1-based
 * answer, <= 0 for none.  res == NULL: nothing per read comes back; else res is exactly what
 * svg_cell_assign_batch returns.  The store grows by reallocation (SVG_E_NOMEM when the device
 * refuses, or past option cell_count_max_mb); a failed call leaves the counter as it was before.
 *
 * svg_cell_counter_finish answers for everything added since create or reset, may be called again,
 * and add / count_batch after it go on accumulating.  counts: ascending (sample, cell, gene), sample
 * s (1-based) at counts[count_first[s-1] .. count_first[s]) (the reference writes hash-iteration
 * order).  want_entries: one svg_cell_umi_entry per distinct (sample, cell, gene, UMI) in step 1's
 * order, sample s at entries[entry_first[s-1] .. entry_first[s]).
 * svg_cell_count_timing (under svg_set_timing) returns and resets the summed milliseconds of:
 * expand, sort + run-length (support count and step 1's order), step 1 lane kernel, step 1 wave
 * kernel, step 2 (sort + flags), count table.
 */
#define SVG_CELL_MAX_UMI        14   /* MAX_UMI_LEN */
#define SVG_CELL_MAX_SAMPLES    255
#define SVG_CELL_MAX_CELLS      (1 << 24)
#define SVG_CELL_UMI_COUNTED    0    /* counts 1 for its (cell, gene) */
#define SVG_CELL_UMI_MERGED     1    /* merged into acceptor_umi in step 1 */
#define SVG_CELL_UMI_LOST       2    /* not the first of its (cell, UMI) section in step 2 */
#define SVG_CELL_UMI_REMOVED    3    /* the first of its section, its support not above the second's */

typedef struct svg_cell_counter svg_cell_counter;

typedef struct svg_cell_count {
	int32_t  sample, cell, gene;
	uint32_t n_umis;
} svg_cell_count;                     /* 16 bytes */

typedef struct svg_cell_umi_entry {
	int32_t  sample, cell, gene;
	uint32_t support;                 /* before step 1 */
	uint32_t support_merged;          /* after step 1 (an acceptor's has grown) */
	uint32_t outcome;                 /* SVG_CELL_UMI_* */
	char     umi[SVG_CELL_MAX_UMI];            /* zero to the end */
	char     acceptor_umi[SVG_CELL_MAX_UMI];   /* SVG_CELL_UMI_MERGED only, else zero */
} svg_cell_umi_entry;                 /* 52 bytes */

typedef struct svg_cell_counts {
	uint32_t n_samples, umi_length;
	uint64_t n_counts, n_entries;
	svg_cell_count *counts;
	uint64_t *count_first;            /* [n_samples + 1] */
	uint64_t *removed_umis;           /* [n_samples] */
	svg_cell_umi_entry *entries;      /* NULL without want_entries */
	uint64_t *entry_first;            /* [n_samples + 1] */
	uint64_t dropped_no_sample, dropped_no_cell;
} svg_cell_counts;

int  svg_cell_counter_create(svg_index *idx, int umi_length, int n_samples, svg_cell_counter **out);
void svg_cell_counter_free(svg_cell_counter *c);
int  svg_cell_counter_reset(svg_cell_counter *c);
int  svg_cell_counter_add(svg_cell_counter *c, const int32_t *sample, const int32_t *cell, const int64_t *gene,
                          const char *umi_text, uint64_t n);
int  svg_cell_count_batch(svg_index *idx, const svg_cell_align_params *p, const svg_packed_reads *reads,
                          const svg_packed_reads *barcodes, const svg_packed_reads *umis, const int32_t *sample_no,
                          svg_cell_counter *c, svg_cell_assigned *res);
int  svg_cell_counter_finish(svg_cell_counter *c, int want_entries, svg_cell_counts *out);
void svg_cell_counts_free(svg_cell_counts *out);
int  svg_cell_count_timing(svg_index *idx, double ms[6]);

/*
 * Read names to barcode, UMI and sample number.  In cellCounts every read carries its cell barcode,
 * UMI and sample index in its name: the readers compose it (cell-counts.c:2191-2242 from BCL,
 * "R%011llu:<barcode+UMI>|<their qualities>|<index>|<its qualities>|@RgLater@L%03d"; input-blc.c:
 * 1779-1829 from FASTQ, "R%011lld|<barcode+UMI>|<qualities>|<index>|<qualities>" or
 * "...|input#%04d@L%03d") and cellCounts_vote_and_add_count takes it apart for every written record
 * (:1955-1976) with cellCounts_scan_read_name_str (:1658-1696) and cellCounts_get_sample_id
 * (:1862-1880).  Here the names go in as text (a svg_reads: NUL-free names, offsets, lengths) and the
 * device does that work, one lane per name.
 *
 * The scan, as written: from the name's second character on, '|' separates, and in
 * SVG_CELL_NAMES_BCL mode ':' does too (:1663) -- also a ':' inside the quality text, which a
 * quality '9' becomes under the increment of :2229; this is kept.  Separator 1: the trimmed name
 * length is its position, the barcode starts behind it and the UMI barcode_length further on;
 * separator 3: the sample text behind it; separator 5: the lane text behind it, past a leading
 * "@RgLater@" (:1679), and the scan stops.  `fields` is the scan's return value.
 * Lane number: the digits from the lane text's second character to the first non-digit (:1967-1971).
 * Sample with a lane text (:1972, cellCounts_get_sample_id): the sheet rows in order, a row whose lane
 * is SVG_CELL_LANE_ALL or the read's; a dual row (index longer than 12, :664) by
 * hamming_dist_ATGC_max1_2p <= 2, a single one by hamming_dist_ATGC_max1 <= 1 (input-blc.c:
 * 1072-1105).  Both compare up to the first character is_ATGC rejects in either string (it accepts N;
 * in the read's text that is the '|' behind the index, or the name's end), so over the shorter of the
 * two; _2p splits that length in halves and allows one mismatch in each; max1 gives up at two.  The
 * first matching row wins, no row gives -1.
 * Sample without a lane text (:1973-1975): a sample text starting "input#" takes the four characters
 * behind it as decimal digits, plus 1, as a 1-based sheet line: lines[line - 1], 0 where the line is
 * absent or beyond n_lines.  Any other sample text gives -1 (:1976).  lane is -1 without a lane text.
 *
 * svg_cell_set_samples: rows is sample_barcode_list in its order (sheet_convert_ss_to_arr,
 * :648-668: the caller parses the sheet), index texts of A/C/G/T, 1..SVG_CELL_MAX_INDEX characters
 * (both indexes of a dual row back to back, as :659-663 store them); at most SVG_CELL_MAX_ROWS rows
 * and lines.  A later call replaces everything; n_rows = n_lines = 0 clears it.  SVG_E_ARG: a sample
 * number outside 1..n_samples in a row (0..n_samples in lines), n_samples outside
 * 1..SVG_CELL_MAX_SAMPLES, another character, an empty or over-long index, too many rows.
 *
 * Outside the reference's contract, defined here: status SVG_CELL_NAME_FEW_FIELDS, fewer than 3
 * separators (the reference then reads through a NULL sample text); SVG_CELL_NAME_PAST_END, the
 * barcode or the UMI runs past the name's end; SVG_CELL_NAME_BAD_CHAR, a barcode or UMI character
 * other than A/C/G/T/N.  Such a name is refused: sample_no -1, lane -1, barcode and UMI all A.
 * Characters beyond a name's end read as NUL.  umi_length < 1 (the reference's auto-detection,
 * :1684-1693) is SVG_E_ARG, as are barcode_length outside 1..16 and umi_length above
 * SVG_CELL_MAX_UMI.  A lane number of more than nine digits is outside the contract (int overflow in
 * the reference); here it wraps as unsigned arithmetic.
 *
 * svg_cell_parse_names returns every field per read: barcodes and umis are svg_packed_reads of
 * stride SVG_CELL_NAME_STRIDE (starts NULL, the exception bit meaning N), the layout
 * svg_cell_count_batch takes; `refused` counts the names with a status.  Free with svg_cell_names_free.
 *
 * svg_cell_count_names_batch is svg_cell_count_batch with the names in the place of barcodes, UMIs
 * and sample numbers: the same chunk loop (one body), the parse kernel in front of every chunk, its
 * output read by the barcode kernel, the expand kernel and the tallies while it is in device memory;
 * nothing of it comes to the host.  The barcode length is the whitelist's (no whitelist: SVG_E_ARG,
 * the UMI's place in the name would be unknown), the UMI length is the counter's, and the sheet's
 * n_samples is at most the counter's.  A refused name gives no
 * observation and no tally; it is counted on the device and svg_cell_counter_finish fails with
 * SVG_E_ARG until svg_cell_counter_reset, as for a value outside its key field.
 *
 * svg_cell_counter_tallies: reads_per_sample, mapped_reads_per_sample and assigned_reads_per_sample
 * (:1993-2004; the SampleTable of :4433-4453), n_samples + 1 numbers each, accumulated on the device
 * by svg_cell_count_batch and svg_cell_count_names_batch (not by svg_cell_counter_add, which sees no
 * records) and cleared by reset.  They count calls of cellCounts_vote_and_add_count, not reads:
 * cellCounts_select_and_write_alignments (:2700-2716) calls the writer once per record with
 * this_multi_mapping_i = reporting_this_alignment_no + 1, and since the records with a score > 0
 * sort first and reporting_multi_alignment_no counts them, the records of a read are numbered
 * 1, 2, ... without a gap; a read without a record gets one call with reporting_index -1.  A record
 * whose position locate_gene_position does not place (contig -1) is turned into that same unmapped
 * call at :2067/:2087 (reporting_index -1, nhits 0, this_multi_mapping_i 0), record by record.  So
 * with sample_no > 0: reads[sample_no - 1] grows by the read's records (1 without any); mapped by 1
 * if the read's first record has a contig; assigned by 1 if that record's nhits (after :1982) is
 * above 0.  A second record never counts as mapped, so a read whose first record has contig -1 is
 * not mapped whatever follows.  With sample_no <= 0 the calls go to reads[n_samples]; mapped and
 * assigned have nothing there.  A sample number above n_samples is tallied nowhere.
 * svg_cell_names_timing (under svg_set_timing) returns and resets the parse kernel's milliseconds.
 */
#define SVG_CELL_NAMES_BCL        0    /* GENE_INPUT_BCL: ':' separates too */
#define SVG_CELL_NAMES_FASTQ      1    /* GENE_INPUT_SCRNA_FASTQ */
#define SVG_CELL_LANE_ALL         99999   /* LANE_FOR_ALL_LANES */
#define SVG_CELL_MAX_INDEX        32
#define SVG_CELL_MAX_ROWS         65536
#define SVG_CELL_NAME_STRIDE      32
#define SVG_CELL_NAME_OK          0
#define SVG_CELL_NAME_FEW_FIELDS  1
#define SVG_CELL_NAME_PAST_END    2
#define SVG_CELL_NAME_BAD_CHAR    3

typedef struct svg_cell_sample_row {
	int32_t lane;                     /* or SVG_CELL_LANE_ALL */
	int32_t sample_no;                /* 1-based */
	const char *index;                /* NUL-terminated */
} svg_cell_sample_row;

typedef struct svg_cell_names {
	uint64_t n_reads, refused;
	int32_t *fields, *trimmed_len, *lane, *sample_no;
	uint32_t *status;                 /* SVG_CELL_NAME_* */
	svg_packed_reads barcodes, umis;  /* stride SVG_CELL_NAME_STRIDE */
} svg_cell_names;

int  svg_cell_set_samples(svg_index *idx, const svg_cell_sample_row *rows, uint64_t n_rows, const int32_t *lines, uint64_t n_lines,
                          int n_samples);
int  svg_cell_parse_names(svg_index *idx, const svg_reads *names, int mode, int barcode_length, int umi_length, svg_cell_names *out);
void svg_cell_names_free(svg_cell_names *out);
int  svg_cell_count_names_batch(svg_index *idx, const svg_cell_align_params *p, const svg_packed_reads *reads, const svg_reads *names,
                                int mode, svg_cell_counter *c, svg_cell_assigned *res);
int  svg_cell_counter_tallies(svg_cell_counter *c, uint64_t *reads, uint64_t *mapped, uint64_t *assigned);
int  svg_cell_names_timing(svg_index *idx, double *ms);

/*
 * Fragile junction voting of subjunc reads longer than 160 bases (core_fragile_junction_voting,
 * core-junction.c:5151-5422; do_voting runs it for every index block, strand and read end,
 * core.c:3138-3142).  The read (strand 0: as fetched after the -S reversal, strand 1: its
 * reverse_read) is cut into ~60-base windows; each window is voted with gehash_go_q
 * (sorted-hashtable.c:515-933: every item of the key's equal-key run from the first one, the
 * go_X tally without shift-indel rounds, tolerance 5) over subreads every 3.00001 bases, then:
 *   - every slot with the top vote count whose indel recorder has a second section is reported
 *     (svg_fragile_slot) -- the reference aligns those on the host (core_dynamic_align) into
 *     indel events;
 *   - select_best_vote + core_select_best_matching_halves pick a second half, and
 *     core13_test_donor (GT..AG / CT..AC donors, 17-base match windows) decides whether the
 *     window supports a junction (small_side, large_side, is_GTAG).
 * svg_fragile_batch runs all of it on the GPU for a batch (host buffers, synchronous; reads as
 * svg_vote_batch takes them, p must be subjunc parameters); the result arrays are owned by the
 * library until svg_fragile_free.  The events are made on the host by svg_events_add_batch2
 * (include/subread_events.h), in the reference's order.
 */
typedef struct svg_fragile_window {
	uint32_t read;             /* read (pair) number in the batch */
	uint8_t  block;            /* index block */
	uint8_t  strand;           /* 0: the read as fetched, 1: reverse_read of it */
	uint8_t  end;              /* 0: R1, 1: R2 */
	uint8_t  window;           /* window number */
	uint16_t start, length;    /* window_cursor and read_len of the window */
	uint8_t  junction;         /* 1: core13_test_donor accepted a split point */
	uint8_t  gtag;             /* its is_GTAG */
	uint16_t n_slots;          /* reported slots: slots[first_slot .. first_slot + n_slots) */
	uint32_t small_side;       /* junction event: min(split + pos1, split + pos2) - 1 */
	uint32_t large_side;       /*                 max(split + pos1, split + pos2) */
	uint32_t first_slot;
} svg_fragile_window;          /* 28 bytes */

typedef struct svg_fragile_slot {
	uint32_t position;         /* the slot's voting position */
	int16_t  rec[9];           /* indel_recorder[0..8], zero after the first empty section */
	uint16_t _pad;
} svg_fragile_slot;            /* 24 bytes */

typedef struct svg_fragile_result {
	uint64_t n_windows, n_slots;
	svg_fragile_window *windows;   /* (block, read, strand, end, window) order: do_voting's */
	svg_fragile_slot *slots;       /* window by window, each window's in row-major slot order */
} svg_fragile_result;

int  svg_fragile_batch(svg_index *idx, const svg_params *p, const svg_reads *r1, const svg_reads *r2,
                       svg_fragile_result *out);
void svg_fragile_free(svg_fragile_result *r);

/* Per-batch statistics of the last svg_vote_batch* call on this handle
 * (filled only after svg_set_stats(idx,1)); used for the algorithmic-byte roofline. */
typedef struct svg_batch_stats {
	uint64_t probes;             /* gehash_go_X calls                         */
	uint64_t bucket_items;       /* sum of items in the probed buckets        */
	uint64_t hits;               /* sum of equal-key run lengths              */
	uint64_t results;            /* mapping records with selected_votes > 0   */
	uint64_t deferred;           /* single-end align: reads that left the lane-per-read
	                                path and were voted by the wave-per-read kernel */
} svg_batch_stats;
int svg_set_stats(svg_index *idx, int enable);

/* Upper bound of read lengths passed to svg_vote_batch_device on this handle
 * (default 256; svg_vote_batch measures its own batch).  A tighter bound lets
 * the library pick a kernel variant with smaller probe tables and higher
 * occupancy.  A read that needs more subread probes than the bound provides
 * gets zeroed records and raises the handle's sticky device error, which
 * svg_device_status() reports as SVG_E_ARG (svg_vote_batch checks it itself). */
int svg_set_max_read_length(svg_index *idx, int max_len);
/* Waits for the work queued on the handle and returns 0, or SVG_E_ARG (message in
 * svg_last_error) when a read since the previous check violated the read-length
 * bound; clears the error.  Calls on one handle are ordered on the device even
 * when they are given different streams. */
int svg_device_status(svg_index *idx);
int svg_get_stats(const svg_index *idx, svg_batch_stats *out);

/* Per-kernel device time (diagnostics / roofline): while enabled, every probe_kernel
 * and vote_kernel launch is bracketed by HIP events on its stream.  svg_get_timing
 * waits for the last recorded event and returns the summed milliseconds and launch
 * counts since svg_set_timing(idx, 1). */
int svg_set_timing(svg_index *idx, int enable);
int svg_get_timing(svg_index *idx, double *probe_ms, double *vote_ms, int *probe_launches, int *vote_launches);
/* The same per kernel: ms[k] / launches[k] for k = 0 probe_kernel, 1 vote_kernel (wave per
 * read), 2 gather_kernel, 3 lane_kernel (lane per read; single-end align).  vote_ms of
 * svg_get_timing is the sum of kinds 1-3. */
int svg_get_kernel_timing(svg_index *idx, double ms[4], int launches[4]);

const char *svg_last_error(void);
int svg_abi_version(void);
/* Expansion worker threads the host entry points use: the "host_threads" option if set, else
 * the CPUs this process may run on (affinity mask capped by the cgroup CPU quota) divided by
 * LOCAL_WORLD_SIZE (one rank per GPU on the node), clamped to 2..12. */
int svg_host_threads(void);

/* NUMA placement of the host side.  svg_host_placement: the NUMA node of `device`'s
 * PCIe function (-1 unknown) and how many CPUs of that node this process may run on; the host
 * entry points pin their expansion workers to those CPUs (when there are any) and take their
 * pinned staging pages from that node.  svg_host_alloc: pinned host memory whose pages come from
 * the node of idx's GPU -- for the caller's reads and records, which the workers and the copy
 * engines touch at ~100 GB/s per rank; release with svg_host_free.  svg_cpulist_parse parses a
 * sysfs cpulist ("0-15,64-79") into a byte mask of `max` entries and returns the CPUs it set. */
int  svg_host_placement(int device, int *node, int *cpus_on_node);
int  svg_host_alloc(svg_index *idx, size_t bytes, void **out);
void svg_host_free(void *p);
int  svg_cpulist_parse(const char *list, uint8_t *mask, int max);

/*
 * Process-wide implementation options.  The library reads no environment variable of its own
 * (only torchrun's LOCAL_WORLD_SIZE, to size host thread pools): tests and tuning set these
 * explicitly.  No option changes a record -- every setting selects among exact implementations
 * of the same reference behaviour (probe images, kernel paths, chunk and sub-batch sizes, pool
 * sizes) or turns on diagnostics printed to stderr.  Names (value 0 / -1 = the default):
 *   host_threads, host_sub      expansion workers; reads per host sub-batch
 *   chunk, overlap              reads per probe-record chunk; 1/0 force the two-stream chunk pipeline
 *   lane                        1 lane kernels + deferral (default), 2 defer every read to the
 *                               wave kernel, 3 no lane kernels (wave kernel only)
 *   lane_unfused                separate gather kernel
 *   lane_bins                   count bins of the fused lane path: 0 lists by heavier strand and
 *                               its count (default), 1 by the larger strand count alone
 *   lane_cap, lane_pe_cap, lane_pairs, lane_mid   lane-path capacities (candidates, pairs)
 *   no_bcode, no_khash, khash64, no_bline, no_compact, kinline, khash_probe, probe_v1,
 *   no_window, probe_colmajor   probe images / probe kernel variants picked at index load
 *   wave_cap                    resident wave-kernel blocks per CU beside the next chunk
 *   probe_cap                   probe line kernel grid, blocks per CU (default 32)
 *   wave_cus, lane_cus_excl     CU masks of the device's streams (read when they are created, at
 *                               the first index load): the wave-kernel stream on CUs 0..wave_cus-1,
 *                               the probe / lane stream on the others with lane_cus_excl 1
 *   host_ramp                   host-buffer entries: sub-batches ramped at both ends (default 1)
 *   host_slots                  device slots of the chunk pipeline, 2 (default) or 3
 *   wave_static                 eighths (0-8) of a chunk's deferred reads the wave kernel deals
 *                               out statically before its work counter (default 6 single-end,
 *                               0 pairs)
 *   keys_literal, long_probes   svg_probe_keys / svg_long_vote_batch variants
 *   cell_count_max_mb           the most device memory a svg_cell_counter's observations may take
 *                               (SVG_E_NOMEM beyond; 0: what the device gives)
 *   debug, pipe_debug, long_debug  diagnostics on stderr
 * svg_set_option returns SVG_E_ARG for an unknown name; svg_get_option returns the current value
 * (0 for an unknown name). */
int     svg_set_option(const char *name, int64_t value);
int64_t svg_get_option(const char *name);

/*
 * Index builder (replaces subread-buildindex for a single-block index,
 * index-builder.c:1014-1306): writes <prefix>.00.b.tab/.00.b.array/.reads/
 * .files/.log byte-identical (tab/array/reads) to the reference.
 *   gap 1 = full index (-F), 3 = gapped (default); memory_mb = -M (8000);
 *   force_one_block = -B; repeat_threshold = -f (100).
 */
int svg_build_index(const char *fasta, const char *prefix, int gap, int memory_mb,
                    int force_one_block, int repeat_threshold);

/* Seeded synthetic data for tests/benchmarks (genRandomReads counterpart). */
void svg_sim_genome(char *out, uint64_t length, uint64_t seed);
void svg_sim_repeats(char *genome, uint64_t length, uint64_t n_copies, uint32_t element_len,
                     uint32_t n_families, double divergence, uint64_t seed);
int  svg_sim_reads(const char *genome, const uint64_t *ctg_start, const uint32_t *ctg_len,
                   uint32_t n_ctg, uint64_t first, uint64_t n_reads, int len, double sub,
                   double indel_frac, double n_rate, uint64_t seed, char *seq,
                   uint32_t *truth_ctg, uint32_t *truth_pos, uint8_t *truth_strand, int threads);
/* paired-end fragments (test/bench input generator): R1 forward, R2 reverse
 * complement of the fragment end; pairs first..first+n_pairs-1 of the stream. */
int  svg_sim_pairs(const char *genome, const uint64_t *ctg_start, const uint32_t *ctg_len, uint32_t n_ctg,
                   uint64_t first, uint64_t n_pairs, int len, double ins_mean, double ins_sd, int ins_max,
                   double sub, uint64_t seed, char *seq1, char *seq2, int threads);

#ifdef __cplusplus
}
#endif
#endif /* SUBREAD_VOTE_H */
