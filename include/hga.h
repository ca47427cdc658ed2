/* hga.h — C ABI of the MI355X k-mer hot path (libhga.so).
 *
 * The reference has no FFI; its seams are a process boundary and an in-process C++
 * API.  Every entry point below names the reference interface it replaces
 * (paths relative to the reference tree).  Plain pointers and sizes only; no
 * exception crosses the ABI; every call returns an hga_status and
 * hga_last_error() returns a thread-local message for the last failure.
 *
 * Threading: one hga_ctx owns one HIP stream on one device.  A ctx is not
 * thread-safe; several ctx per device are allowed.  Host buffers passed in are
 * caller-owned and may be freed as soon as the call returns.  Buffers the library
 * allocates for the caller are released with hga_free().
 */
#ifndef HGA_H
#define HGA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hga_ctx hga_ctx;

typedef enum hga_status {
    HGA_OK = 0,
    HGA_ERR_INVALID = 1, /* bad argument (k out of range, unknown file index, ...)  */
    HGA_ERR_HIP = 2,     /* a HIP runtime call failed                                */
    HGA_ERR_OOM = 3,     /* device or host allocation failed                         */
    HGA_ERR_STATE = 4,   /* call out of order (e.g. select before count_run)         */
    HGA_ERR_COMM = 5     /* RCCL failure                                             */
} hga_status;

/* Thread-local text of the last error ("" if none). */
const char* hga_last_error(void);
/* Frees any buffer the library returned through an out-pointer. */
void hga_free(void* p);
/* Number of visible HIP devices. */
hga_status hga_device_count(int* n);
/* Library/kernel build identification string (static). */
const char* hga_version(void);

hga_status hga_ctx_create(hga_ctx** out, int device);
hga_status hga_ctx_destroy(hga_ctx* ctx);

/* ------------------------------------------------------------------------------
 * Counting — replaces reference seam #1 (the per-file
 *   popen("./occurrences/run_jellyfish.sh <reads> <k> <sorted>")  of
 *   src/occurrences/JellyfishOccurrenceReader.cpp:19-24, i.e. `jellyfish bc/count -C
 *   --bc`, `dump -c` and `LC_ALL=C sort`, src/occurrences/run_jellyfish.sh:3-6)
 * and both k-way merge passes of seam #2 (JellyfishOccurrenceReader::get_next_kmer,
 *   get_specificity, export_kmers; src/occurrences/JellyfishOccurrenceReader.cpp:63-135).
 * ------------------------------------------------------------------------------ */

/* Starts a counting session: k in [1,32], n_files in [1,64] (one file = one haplotype,
 * README.md:36).  Replaces JellyfishOccurrenceReader(paths, k)
 * (src/occurrences/JellyfishOccurrenceReader.h:32).
 * Reads (hga_count_add) are counted with one counter per file in every slot of the count kernel's
 * table, which holds up to 14 files (15 when the key bits below the bucket bits number at most 31);
 * with more files hga_count_run returns HGA_ERR_INVALID unless every file comes from dump rows
 * (hga_count_add_rows), which are merged without that table. */
hga_status hga_count_begin(hga_ctx* ctx, int k, uint32_t n_files);

/* Appends sequence bytes of file `file` (copied to HBM).  `seq` holds whole reads
 * separated by any byte that is not A/C/G/T (either case), e.g. '\n'; windows
 * containing such a byte are not counted (jellyfish semantics).  May be called
 * several times per file; a read must not straddle two calls. */
hga_status hga_count_add(hga_ctx* ctx, uint32_t file, const char* seq, uint64_t n_bytes);

/* Appends the reads of a FASTA / FASTQ file given as its raw bytes: the file is parsed on the device.
 * `bytes` holds whole records of one file: the whole file, or a piece cut at a record start; at most
 * 2^32 - 1 bytes per call (HGA_ERR_INVALID beyond).  What is appended is what jellyfish's reader hands
 * to the counter for these bytes (`jellyfish count` over the file, src/occurrences/run_jellyfish.sh:3-6):
 * the sequence of every record, records separated by one '\n'.  Lines are std::getline's ('\n' ends a
 * line, a last line without one counts, '\r' is an ordinary byte); with `first` the first non-empty line:
 *   layout 0  no non-empty line: nothing appended, 0 records;
 *   layout 1  FASTA: `first` starts with '>'.  Every non-empty line starting with '>' is a header (one
 *             '\n', none for the first), every other line is sequence (its bytes, also when it starts
 *             with '@' or '+'), empty lines add nothing; records = headers;
 *   layout 2  FASTQ in 4-line records: `first` is line 0 and starts with '@', the line count is a multiple
 *             of 4, and every record has an '@' line, a sequence line not starting with '+', a '+' line
 *             and a quality line as long as the sequence; the sequence lines joined by '\n';
 *   layout 3  anything else (multi-line FASTQ, ...): nothing is appended, the ctx is exactly as before the
 *             call, HGA_OK is returned and the caller parses these bytes on the host.
 * For layouts 0-2 the ctx is left exactly as hga_count_add(the stream of these bytes) would leave it: the
 * same growth, the same single '\n' between calls.  Calls may be repeated per file and mixed with
 * hga_count_add and hga_count_add_rows, with or without a communicator.  Synchronous; `bytes` may be
 * pageable memory and is not read after the return.  The parser's device buffers (the raw bytes and
 * 4 bytes per line) are kept between calls and released by hga_count_run.
 * info->lines is filled for every layout, records and seq_bytes (the bytes appended, without the
 * separator between calls) for layouts 1 and 2.
 * HGA_ERR_STATE before hga_count_begin; HGA_ERR_INVALID for a bad file index, NULL bytes with
 * n_bytes > 0, NULL info. */
typedef struct hga_ingest_info {
    uint32_t layout;
    uint32_t reserved;
    uint64_t records, lines, seq_bytes;
} hga_ingest_info;
hga_status hga_count_add_file(hga_ctx* ctx, uint32_t file, const char* bytes, uint64_t n_bytes,
                              hga_ingest_info* info);
/* The resident stream of a file, as hga_count_add / hga_count_add_file left it (hga_free). */
hga_status hga_count_seq(hga_ctx* ctx, uint32_t file, char** bytes, uint64_t* n);
/* Input bytes per workgroup tile of the parser's kernels (the sizes at which the tests change paths). */
uint32_t hga_ingest_tile(void);

/* Adds file `file`'s rows from an existing "<reads>_<k>-mers_sorted" dump instead of its
 * reads: the reference skips jellyfish for a file whose dump exists and merges the dump
 * verbatim (src/occurrences/JellyfishOccurrenceReader.cpp:19-24 and the reader's
 * get_next_kmer, :63-86).  keys = canonical codes (< 4^k, any order), counts >= 1
 * (rows with count 0 are ignored); copied, may be freed on return.  hga_count_run then
 * counts the files given by reads (with the per-file drop) and sums in the dump rows
 * without dropping any.  A file may have both reads and rows; their counts add. */
hga_status hga_count_add_rows(hga_ctx* ctx, uint32_t file, const uint64_t* keys, const uint32_t* counts,
                              uint64_t n);

/* Runs the device pipeline on everything added: canonical k-mers, per-file exact
 * counts, per-file drop of k-mers whose count is < min_per_file (2 = jellyfish
 * `--bc`), merge across files.  May be re-run (bench).  Asynchronous: the launches are
 * queued and the call returns; the run's own failures (level-1 pool, unsplittable bucket,
 * row capacity) are reported by the next count call that consumes its rows
 * (hga_count_spec_hist, _select*, _rows, _dump, _get_stats, the exchange calls), which
 * then fails with that status.  A run nobody consumed is discarded, errors included, by the
 * next hga_count_run or hga_count_add_rows (whose rows replace it). */
hga_status hga_count_run(hga_ctx* ctx, uint32_t min_per_file);

typedef struct hga_count_stats {
    uint64_t instances;      /* k-mer windows counted (all files)                  */
    uint64_t distinct_rows;  /* merged rows present after the per-file drop       */
    uint64_t bytes;          /* sequence bytes resident on the device              */
    uint32_t buckets;        /* hash buckets used by the binning pass              */
    uint32_t max_split;      /* largest sub-pass split any bucket needed           */
} hga_count_stats;
hga_status hga_count_get_stats(hga_ctx* ctx, hga_count_stats* out);

/* Key-range passes: inputs whose work buffers would not fit the device are counted in P passes,
 * each a complete count of the keys whose hashed value starts with the pass's log2 P bits, in
 * buffers of about 1/P of the size; the reads stay resident (1 B/base) and are read P times.  The
 * results (rows, dumps, histogram, export) are those of one pass.
 * passes: 0 = choose from budget_bytes; >= 1 = exactly that many (rounded up to a power of two, clamped
 * to 256 and to what k allows: 2k - log2 P >= 7, two passes at most for k <= 3).
 * budget_bytes: device bytes the count's work buffers and rows may use; 0 = free device memory at
 * hga_count_run (hipMemGetInfo) less a margin.  Default (never called): as today when one pass fits
 * the free memory, else the smallest P that does.
 * A pass's buffers hold 1.25x its expected share of the instances; with budget_bytes > 0 that margin
 * grows as far as the budget allows, up to the whole input.  A key range heavier than that (one k-mer
 * that is a large share of the input: more passes do not split a key) makes the next consuming call
 * fail with HGA_ERR_OOM, the text naming passes and budget; so does a request that cannot fit
 * budget_bytes at any P (at hga_count_run).  When the rows' full capacity (bases / min_per_file) does
 * not fit, they get what the budget leaves (row capacity exceeded -> HGA_ERR_OOM as ever).
 * Not supported on a ctx with a communicator: hga_count_run with P > 1 returns HGA_ERR_STATE. */
hga_status hga_count_set_passes(hga_ctx* ctx, uint32_t passes, uint64_t budget_bytes);
/* Host arithmetic only: the bytes hga_count_run would request for everything added so far, at
 * `passes` (0: the P the budget set by hga_count_set_passes chooses; one pass without a budget) under
 * that budget.  The scans' scratch (a few KB) is not included. */
hga_status hga_count_estimate(hga_ctx* ctx, uint32_t min_per_file, uint32_t passes, uint64_t* bytes);
typedef struct hga_count_pass_stats {
    uint32_t passes;            /* passes the last run used (after clamping)            */
    uint32_t pad;
    uint64_t work_bytes;        /* bytes the run requested for work buffers + rows      */
    uint64_t max_pass_instances;
    uint64_t min_pass_instances;
} hga_count_pass_stats;
hga_status hga_count_get_pass_stats(hga_ctx* ctx, hga_count_pass_stats* out);

/* Specificity histogram — JellyfishOccurrenceReader::get_specificity
 * (src/occurrences/JellyfishOccurrenceReader.cpp:88-108): for every merged row,
 * spec = first threshold > ((double)max_f c_f / (double)Σ c_f) * 100 and
 * result[spec][Σc] += 1.  thr must be ascending; every row must fall below the last
 * threshold.  Output: *triples = malloc'ed int64 [3 * *n]: (threshold index, total,
 * unique k-mer count), ordered by threshold then total (std::map order);
 * thresholds with no rows produce no triple. */
hga_status hga_count_spec_hist(hga_ctx* ctx, const double* thr, uint32_t n_thr,
                               int64_t** triples, uint64_t* n);

/* Export selection — JellyfishOccurrenceReader::export_kmers
 * (src/occurrences/JellyfishOccurrenceReader.cpp:110-135) with percent >= 1: the
 * canonical codes of all merged rows with lower <= Σc <= upper, ascending
 * (== the reference's LC_ALL=C string order for fixed k), and the number of them
 * present in exactly one file (:128-130).  *keys malloc'ed (hga_free).
 * Sampling for percent < 1 is host work on this output (see host/jf_occurrences). */
hga_status hga_count_select(hga_ctx* ctx, int64_t lower, int64_t upper, uint64_t** keys,
                            uint64_t* n, uint64_t* n_discriminative);
/* Same, plus one byte per key: 1 if that k-mer is present in exactly one file.  The
 * host needs the flags when it samples with percent < 1 (:128-130).  *keys and
 * *discriminative are malloc'ed (hga_free). */
hga_status hga_count_select_ex(hga_ctx* ctx, int64_t lower, int64_t upper, uint64_t** keys,
                               uint8_t** discriminative, uint64_t* n, uint64_t* n_discriminative);
/* Same, leaving the sorted keys on the device (bench / chained use). */
hga_status hga_count_select_device(hga_ctx* ctx, int64_t lower, int64_t upper,
                                   uint64_t* n, uint64_t* n_discriminative);

/* All merged rows, ascending by code: keys[rows], counts[rows * n_files] row-major.
 * This is the stream JellyfishOccurrenceReader::get_next_kmer yields. */
hga_status hga_count_rows(hga_ctx* ctx, uint64_t** keys, uint32_t** counts, uint64_t* rows);

/* One file's dump: rows with count >= min_per_file in that file, ascending — the
 * content of "<reads>_<k>-mers_sorted" (run_jellyfish.sh:5-6). */
hga_status hga_count_dump(hga_ctx* ctx, uint32_t file, uint64_t** keys, uint32_t** counts,
                          uint64_t* rows);

/* Multi-GPU owner exchange (the reference is single-process).  Each rank
 * counts its shard with hga_count_run(ctx, 1), so no per-file singleton is dropped before
 * the global sum, then:
 *   hga_count_partition  writes the rank's merged rows grouped by owner into caller-owned
 *     DEVICE buffers keys_out[rows] and counts_out[rows * n_files] (row-major), owner o first
 *     covering codes in [splitters[o-1], splitters[o]) (n_owners-1 ascending splitters, host
 *     memory); rows_per_owner[n_owners] (host) receives each owner's slice length.  The
 *     buffers hold hga_count_get_stats().distinct_rows rows.  Returns when they are complete.
 *   (caller) one all-to-all per array over RCCL.
 *   hga_count_merge      takes the rows received by this owner (DEVICE pointers, any order,
 *     at most one row per key per source rank), sums equal keys, applies the per-file drop
 *     (count >= min_per_file, the `--bc` of run_jellyfish.sh:3-6) and makes the result the
 *     ctx's merged rows: spec_hist / select / rows / dump then run on this owner's key range,
 *     ascending, exactly as JellyfishOccurrenceReader.cpp:63-135 would over the whole input. */
hga_status hga_count_partition(hga_ctx* ctx, const uint64_t* splitters, uint32_t n_owners,
                               uint64_t* keys_out, uint32_t* counts_out, uint64_t* rows_per_owner);
hga_status hga_count_merge(hga_ctx* ctx, const uint64_t* keys, const uint32_t* counts, uint64_t n,
                           uint32_t min_per_file);

/* Packed form of the same exchange (half the bytes): one u64 per row piece, key in the low 2k
 * bits, file f's count in the `bits` bits above it (bits = (64 - 2k) / n_files, 0 when below 4
 * or n_files > 8: use the wide form).  A row whose count exceeds 2^bits - 1 is sent as several
 * pieces with the same key; the owner's merge sums them.
 *   hga_count_partition_packed: pieces grouped by owner into DEVICE buffer out[capacity];
 *     pieces_per_owner[n_owners] and *total (host).  If *total > capacity nothing is written
 *     and HGA_ERR_OOM is returned (call again with room for *total).
 *   hga_count_merge_packed: the pieces this owner received (DEVICE pointer, any order). */
hga_status hga_count_pack_bits(hga_ctx* ctx, int* bits);
hga_status hga_count_partition_packed(hga_ctx* ctx, const uint64_t* splitters, uint32_t n_owners,
                                      uint64_t* out, uint64_t capacity, uint64_t* pieces_per_owner,
                                      uint64_t* total);
hga_status hga_count_merge_packed(hga_ctx* ctx, const uint64_t* pieces, uint64_t n,
                                  uint32_t min_per_file);

/* ------------------------------------------------------------------------------
 * Multi-GPU counting inside the library (SURVEY.md §8(b) `hga_comm_init`, §8(e)).  The
 * reference is single-process; this replaces its one jellyfish run per file with one rank per
 * GPU, each counting a contiguous shard of every file.  One hga_ctx per rank: one process per
 * GPU, or one thread per GPU in one process (bin/jf_occurrences --gpus N).
 *
 *   every rank:  hga_count_begin / hga_count_add (its shard) / hga_count_run(ctx, 1)
 *                hga_count_exchange(ctx, min_per_file)   (collective)
 *   then hga_count_spec_hist / _select / _select_ex / _rows / _dump / _get_stats answer for the
 *   whole input, identically on every rank (collectives: call them on every rank, same order);
 *   hga_count_select_device leaves each owner's sorted slice on its device and returns the global
 *   (n, n_discriminative).  Gathered results are the owners' sorted slices merged by key, i.e. the
 *   reference's order (JellyfishOccurrenceReader.cpp:63-135).  A later hga_count_run makes the ctx
 *   local again until the next exchange.  With a communicator attached, hga_count_run(ctx, 1)
 *   already groups its rows for the exchange; local queries before the exchange still work.
 * ------------------------------------------------------------------------------ */
#define HGA_UNIQUE_ID_BYTES 128
/* RCCL unique id (ncclGetUniqueId): create on one rank, hand the bytes to all ranks. */
hga_status hga_comm_unique_id(void* id /* HGA_UNIQUE_ID_BYTES */);
/* RCCL communicator over xGMI for this ctx's device (ncclCommInitRank; blocks until every rank
 * joined).  Exchanges are enqueued on the ctx stream. */
hga_status hga_comm_init(hga_ctx* ctx, const void* unique_id, int rank, int nranks);

/* Host-staged transport supplied by the caller (gloo, MPI, sockets, threads of one process).
 * alltoallv is collective: every rank calls it in the same order; send_bytes[p] bytes at send[p]
 * go to rank p, recv_bytes[p] bytes from rank p land at recv[p] (host memory; the library stages
 * device data).  Returns 0 on success. */
typedef struct hga_transport {
    void* user;
    int (*alltoallv)(void* user, const void* const* send, const uint64_t* send_bytes, void* const* recv,
                     const uint64_t* recv_bytes);
} hga_transport;
hga_status hga_comm_init_host(hga_ctx* ctx, int rank, int nranks, const hga_transport* transport);
/* This ctx's rank and rank count (0 and 1 without a communicator). */
hga_status hga_comm_info(hga_ctx* ctx, int* rank, int* nranks);
/* Gathered lists on one rank only (the export and the dumps to one writer, as the
 * reference's single export_kmers pass writes them, JellyfishOccurrenceReader.cpp:110-135): after it,
 * hga_count_select / _select_ex / _rows / _dump still run on every rank (collectives), but only rank
 * `root` receives the list; the other ranks get an empty one (*n, *n_discriminative, *rows = 0).  One
 * copy crosses the ranks instead of P.  root = -1 (the default): every rank gets the whole list. */
hga_status hga_comm_set_root(hga_ctx* ctx, int root);
hga_status hga_comm_destroy(hga_ctx* ctx);

/* Owner exchange after hga_count_run(ctx, 1) on every rank: owners hold ranges of a hash of the
 * k-mer; one all-to-all-v of packed row pieces (one u64 each) and one of per-bucket counts, owner
 * merge with the per-file drop count >= min_per_file (jellyfish --bc, run_jellyfish.sh:3-6); rows
 * that do not pack go as (key, counts) rows to canonical-code ranges. */
hga_status hga_count_exchange(hga_ctx* ctx, uint32_t min_per_file);

/* ------------------------------------------------------------------------------
 * SDK lookup — replaces the per-read loop of ReadClusteringEngine::construct_indices
 * (src/clustering/ReadClusteringEngine.cpp:234-299).  The host keeps SDK loading
 * (src/read_clustering.cpp:18-33) and the KmerID assignment (iteration order of the
 * std::unordered_set, ReadClusteringEngine.cpp:237-241).
 * ------------------------------------------------------------------------------ */

/* Uploads the SDK set: keys_in_id_order[i] is the canonical code of KmerID i. */
hga_status hga_lookup_load(hga_ctx* ctx, int k, const uint64_t* keys_in_id_order, uint32_t n);

/* Uploads reads in reader order as a CSR: read i = bases[offsets[i], offsets[i+1]).
 * Read i has ReadID first_read_id + i (SequenceRecordIterator IDs are consecutive,
 * 1-based, src/common/SequenceRecordIterator.cpp:27,168). */
hga_status hga_lookup_set_reads(hga_ctx* ctx, const char* bases, const uint64_t* offsets,
                                uint64_t n_reads, uint32_t first_read_id);

/* Runs the lookup and builds every index on the device. */
hga_status hga_lookup_run(hga_ctx* ctx);

typedef struct hga_lookup_sizes {
    uint64_t n_reads;
    uint64_t windows;   /* k-mer windows scanned                                       */
    uint64_t hits;      /* H: windows whose canonical code is an SDK                   */
    uint64_t firsts;    /* U: distinct (read, KmerID) pairs                            */
    uint64_t reads_hit; /* reads with >= 1 hit (the ReadComponents created)            */
    uint32_t n_sdk;     /* K                                                           */
} hga_lookup_sizes;
hga_status hga_lookup_get_sizes(hga_ctx* ctx, hga_lookup_sizes* out);

/* Caller-allocated output arrays (any may be NULL to skip):
 *  hit_ptr[n+1], hit_kid[H], hit_pos[H]: per read, hits in window order with the
 *      end-exclusive position (KmerIterator::position_in_sequence);
 *  sorted_kid[H]: per read, KmerIDs ascending with duplicates
 *      (ReadComponent::discriminative_kmer_ids, ReadClusteringEngine.cpp:262-272);
 *  first_ptr[n+1], first_kid[U], first_pos[U]: ReadMetaData::kmer_positions
 *      (first occurrence wins, :267) listed by ascending KmerID;
 *  kci_ptr[K+1], kci_read[H]: kmer_component_index, per KmerID the ReadIDs, one per
 *      occurrence, ascending (:262-263, 282-284). */
typedef struct hga_lookup_result {
    uint64_t* hit_ptr;
    uint32_t* hit_kid;
    uint32_t* hit_pos;
    uint32_t* sorted_kid;
    uint64_t* first_ptr;
    uint32_t* first_kid;
    uint32_t* first_pos;
    uint64_t* kci_ptr;
    uint32_t* kci_read;
} hga_lookup_result;
hga_status hga_lookup_fetch(hga_ctx* ctx, const hga_lookup_result* out);

/* The lookup in read batches: the same result as hga_lookup_set_reads + hga_lookup_run on the
 * concatenated reads, with the scan's device memory (about 5.5 B per base one-shot) bounded by the
 * largest batch instead of the read set.  After hga_lookup_finish every consumer of a lookup result
 * (hga_lookup_get_sizes / _fetch / _gather, hga_connections_*, hga_components_*, hga_spanning_forest*,
 * hga_tree_tails, hga_read_overlaps, hga_connections_quality) works as after hga_lookup_run.
 *
 * hga_lookup_begin opens a session (HGA_ERR_STATE before hga_lookup_load); it invalidates what
 * hga_lookup_run invalidates and releases the read buffers of an earlier hga_lookup_set_reads.  A second
 * begin abandons the open session and starts again.
 * hga_lookup_add_reads appends a CSR of whole reads (offsets[0] == 0, non-decreasing, as
 * hga_lookup_set_reads): read i of this call has ReadID first_read_id + (reads added before) + i; all
 * reads of a session number fewer than 2^32.  A batch of no reads, of empty reads only, or without a
 * hit is legal.  On return the caller's buffers may be reused; the batch's kernels need not have
 * finished, and an error of theirs is reported by a later hga_lookup_add_reads or by hga_lookup_finish.
 * hga_lookup_finish builds the indices over all hits and closes the session.  No reads stay resident:
 * hga_hll_registers and hga_lookup_run return HGA_ERR_STATE until the next hga_lookup_set_reads.
 * While a session is open, hga_lookup_run / _fetch / _get_sizes / _gather / _load, hga_hll_registers and
 * every consumer of a lookup result return HGA_ERR_STATE (the message names the open session);
 * hga_lookup_set_reads abandons the session and returns to the one-shot path.
 *
 * Device memory of a session: two slots sized by the largest batch seen (hga_lookup_batch_estimate:
 * host arithmetic only, their bytes for batches of at most batch_bases bases and batch_reads reads),
 * and the hit arrays (24 B per hit), grown geometrically with their contents kept. */
hga_status hga_lookup_begin(hga_ctx* ctx, uint32_t first_read_id);
hga_status hga_lookup_add_reads(hga_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_reads);
hga_status hga_lookup_finish(hga_ctx* ctx);
hga_status hga_lookup_batch_estimate(hga_ctx* ctx, uint64_t batch_bases, uint64_t batch_reads,
                                     uint64_t* slot_bytes);
typedef struct hga_lookup_batch_stats {
    uint64_t batches;       /* hga_lookup_add_reads calls of the session                          */
    uint64_t reads;
    uint64_t bases;
    uint64_t slot_bytes;    /* device bytes allocated for both slots at the largest batch seen   */
    uint64_t result_bytes;  /* device bytes of the appended hit arrays (their capacity)          */
    uint64_t regrowths;     /* times the hit arrays were replaced by larger ones, contents kept  */
    uint64_t host_waits;    /* times the host waited for a batch's hit count                     */
} hga_lookup_batch_stats;
/* The open session so far, or the last finished one (HGA_ERR_STATE before any hga_lookup_begin). */
hga_status hga_lookup_get_batch_stats(hga_ctx* ctx, hga_lookup_batch_stats* out);

/* Sharded lookup on a ctx with a communicator: every rank loads the same
 * SDK set (hga_lookup_load), sets its contiguous ReadID range of the reads (hga_lookup_set_reads with
 * first_read_id = the range's first ReadID, ranks in ReadID order) and runs hga_lookup_run; then
 * hga_lookup_gather (collective) replaces the ctx's results with the whole input's index, identical
 * on every rank: hga_lookup_get_sizes / hga_lookup_fetch describe all reads in ReadID order, and
 * kmer_component_index is per KmerID the ranks' lists concatenated in rank order (= ascending, as
 * ReadClusteringEngine.cpp:282-284 leaves it).  hga_connections_run then sees every read; each rank
 * passes its own ReadIDs as pivots (categories, if any, for all reads) and hga_connections_gather
 * (collective) joins the ranks' connections in the reference order (score descending, ties by
 * (pivot, candidate); :331) for hga_connections_fetch.  The next hga_lookup_run returns to the rank's
 * own reads. */
hga_status hga_lookup_gather(hga_ctx* ctx);
hga_status hga_connections_gather(hga_ctx* ctx, uint64_t* n);

/* ------------------------------------------------------------------------------
 * HyperLogLog k-mer cardinality — replaces get_approximate_kmer_count
 * (src/occurrences/KmerAnalysis.cpp:15-38), the estimator behind jf_occurrences' automatic
 * k selection (get_unique_k_length, KmerAnalysis.cpp:41-56; src/jellyfish_occurrences.cpp:40-44).
 * ------------------------------------------------------------------------------ */

/* Registers of hll::HyperLogLog(b) (src/lib/HyperLogLog.hpp:96-106) after add() of the
 * canonical code (8 little-endian bytes, MurmurHash3_x86_32 seed 313) of every KmerIterator
 * window of the reads uploaded with hga_lookup_set_reads.  registers[2^b] (caller-allocated)
 * receive M[index] = max rank; order-independent, so bit-identical to the reference.
 * b in [4, 14] (the reference uses 10); k in [1, 32] ("Kmer size is too big" above 32,
 * KmerIterator.cpp:24-26).  The estimate itself is host arithmetic on these registers. */
hga_status hga_hll_registers(hga_ctx* ctx, int k, uint32_t b, uint8_t* registers);

/* ------------------------------------------------------------------------------
 * Connections — ReadClusteringEngine::get_connections / get_all_connections
 * (src/clustering/ReadClusteringEngine.cpp:301-339) on the one-read components that
 * construct_indices leaves (run after hga_lookup_run, on its device-resident indices).
 * For pivot p and every other read c: score = sum over KmerIDs of (occurrences in p) x
 * (occurrences in c), i.e. the robin_map count of :311-315; pairs with score >= min_score
 * are kept (:318-325), the pivot itself never (:316).
 * ------------------------------------------------------------------------------ */

/* pivots: ReadIDs (the reference's component_ids), or NULL for every read with at least
 *   min_kmers hits (min_kmers = 1: get_all_connections, :335-339; min_kmers = s with
 *   min_score = s: the filter_components(... discriminative_kmer_ids.size() >= s) call
 *   site, :750-751).  A pivot without hits yields nothing.
 * categories: per read of the lookup (read order, n_reads), or NULL.  is_good =
 *   categories[p] == categories[c] when given (the reference's debug mode, :319), else 0.
 * Result order: score descending (std::sort(rbegin, rend), :331); ties, unordered in the
 *   reference, by (pivot, candidate) ascending.  *n = number of connections. */
hga_status hga_connections_run(hga_ctx* ctx, const uint32_t* pivots, uint64_t n_pivots, uint32_t min_kmers,
                               uint64_t min_score, const int32_t* categories, uint64_t* n);
/* Copies the result (caller-allocated, n entries each; any may be NULL): ComponentConnection
 * {component_x_id = x, component_y_id = y, score, is_good}
 * (src/clustering/ReadClusteringEngine.h:127-136). */
hga_status hga_connections_fetch(hga_ctx* ctx, uint32_t* x, uint32_t* y, uint64_t* score, uint8_t* is_good);
/* The same for entries [first, first + count) of the result (clipped to n): run_clustering keeps only the
 * first scaffold_forming_fraction of get_all_connections' sorted list (src/clustering/ReadClusteringEngine.cpp:754-755),
 * so the caller fetches just that prefix. */
hga_status hga_connections_fetch_range(hga_ctx* ctx, uint64_t first, uint64_t count, uint32_t* x, uint32_t* y,
                                       uint64_t* score, uint8_t* is_good);

/* Connection quality — the two histograms plot_connection_quality pipes to the plotting script under -d
 * (src/clustering/ReadClusteringEngine.cpp:19-34 and :102-124), over a whole ordered connection list
 * where it lies: per distinct score, how many counted connections are good and how many bad.
 * List: x == y == score == NULL: the ctx's current ordered connection result, as hga_spanning_forest
 *   reads it (after hga_connections_run, hga_components_connections or hga_connections_gather; n and
 *   is_good are ignored; HGA_ERR_STATE without one).  x, y and score all given: n host rows, copied;
 *   is_good may be NULL (all 0).  The rows must be in result order, score non-increasing (checked on the
 *   host), and every id one of the current lookup's ReadIDs; x[i] == y[i] is legal and counts like any
 *   row.  Otherwise, and for any other NULL mix: HGA_ERR_INVALID with nothing launched.  More than
 *   2^32 - 2 rows: HGA_ERR_INVALID (positions are 32-bit on the device).
 * vertex_class: NULL, or n_reads entries in read order; when given, good = vertex_class[x] ==
 *   vertex_class[y] replaces the stored flag.  (After a merge is_good compares the components' category
 *   sets, which only the host holds: the caller numbers the distinct sets.)
 * per_candidate == 0 (:19-34): every row counts once, under its score and its flag.
 * per_candidate != 0 (:102-124): one count per distinct y, from the row the reference loop keeps.  The
 *   loop replaces its entry only on a strictly larger score and the list is score-descending, so that
 *   is the row at the smallest position among the rows with that y; where scores tie this follows the
 *   result order's (pivot, candidate), the reference's order is unspecified there.  A kept row of score
 *   0 counts as bad whatever its flag: the loop starts from {0, false} and never replaces it (:105-108).
 * Result: three hga_free-able arrays of *n_rows entries: the scores strictly ascending (full 64 bits),
 *   good and bad counts.  A score is listed only if good + bad > 0; *n_rows = 0 for an empty list.
 * Synchronous; HGA_ERR_STATE before hga_lookup_run.  The connection result is only read. */
hga_status hga_connections_quality(hga_ctx* ctx, const uint32_t* x, const uint32_t* y, const uint64_t* score,
                                   const uint8_t* is_good, uint64_t n, int per_candidate,
                                   const int32_t* vertex_class /* n_reads, or NULL */, uint64_t** out_score,
                                   uint64_t** out_good, uint64_t** out_bad, uint64_t* n_rows);
/* Rows per workgroup of its kernels (the sizes at which the tests change paths). */
uint32_t hga_connections_quality_tile(void);

/* ------------------------------------------------------------------------------
 * Read overlaps — ReadClusteringEngine::approximate_read_overlap as get_spanning_tree_tails
 * calls it per spanning-tree edge (src/clustering/ReadClusteringEngine.cpp:491-513), for n
 * read pairs at once on the ctx's current lookup result (the rank's own reads, or the whole
 * input's index after hga_lookup_gather).
 * For ReadIDs x[i], y[i]: S = the KmerIDs both reads hit (the intersection of their distinct
 * first_kid lists; the reference's multiset intersection pairs duplicates, which share one
 * kmer_positions entry, so only the set matters).  shared[i] = |S|; overlap[i] = 0 if S is
 * empty (max_element of an empty range there), else max(max - min of first_pos in x over S,
 * max - min of first_pos in y over S).  x[i] == y[i] is allowed; the result is symmetric.
 * ------------------------------------------------------------------------------ */

/* x, y: host arrays of n ReadIDs in [first_read_id, first_read_id + n_reads), copied; any
 *   other id: HGA_ERR_INVALID with nothing launched.  n == 0 is HGA_OK.
 * overlap, shared: caller-allocated, n entries each; either may be NULL.
 * Synchronous.  HGA_ERR_STATE before hga_lookup_run. */
hga_status hga_read_overlaps(hga_ctx* ctx, const uint32_t* x, const uint32_t* y, uint64_t n,
                             int32_t* overlap /* n, may be NULL */, uint32_t* shared /* n, may be NULL */);

/* ------------------------------------------------------------------------------
 * Merged components — ReadClusteringEngine::merge_components
 * (src/clustering/ReadClusteringEngine.cpp:341-422) and get_connections (:301-333) on the state
 * merges leave.  The component view is created lazily from the ctx's current lookup result (the
 * rank's own reads, or the whole input's index after hga_lookup_gather) and dropped by
 * hga_lookup_load / _set_reads / _run / _gather.  hga_lookup_fetch, hga_connections_run and
 * hga_read_overlaps keep answering for the lookup's own state, before and after merges.
 * An id is a ReadID with at least one hit.  Its current KmerID list is the union it received as
 * the survivor of an earlier merge, else the read's own sorted_kid slice (with duplicates).
 * All calls are synchronous; HGA_ERR_STATE before hga_lookup_run.
 * ------------------------------------------------------------------------------ */

/* One merge_components call (:341-422).  groups: n_groups lists, ids[group_ptr[g] .. group_ptr[g+1]);
 * the first id of a list survives (:364).  Empty and one-member lists are no-ops (:358-363).
 * For every longer list the survivor's current list becomes the sorted distinct union of the members'
 * lists (accumulate_kmer_ids, :340-346, :376).  Then kmer_component_index is edited (:389-414): the removal
 * pairs are one (KmerID, member) per entry of every non-survivor member's list and one per KmerID of the
 * union for the survivor; per KmerID the sorted removals are run against the list with the reference's
 * two-pointer loop, which stops once the removals are exhausted (:400-412) and re-inserts nobody.
 * HGA_ERR_INVALID, with nothing launched and no state changed: an id outside
 * [first_read_id, first_read_id + n_reads), an id without hits in a list of two or more, an id listed
 * twice in the call.  n_groups == 0 is HGA_OK. */
hga_status hga_components_merge(hga_ctx* ctx, const uint64_t* group_ptr, const uint32_t* ids, uint64_t n_groups);

/* get_connections (:301-333) on the current state: score(p, c) = sum over the entries of p's current
 * list (with duplicates) of the occurrences of c in that KmerID's current index list (:311-315); c == p
 * is dropped (:316), pairs with score >= min_score are kept (:318-325).  The result is read through
 * hga_connections_fetch / _fetch_range in their order (score descending, then pivot, then candidate),
 * is_good = 0.  A pivot without hits yields nothing; a pivot outside the lookup's reads is
 * HGA_ERR_INVALID; n_pivots == 0 is HGA_OK; min_score above 32 bits yields nothing, as in
 * hga_connections_run.  Before any merge the result equals hga_connections_run(pivots, 1, min_score, NULL). */
hga_status hga_components_connections(hga_ctx* ctx, const uint32_t* pivots, uint64_t n_pivots,
                                      uint64_t min_score, uint64_t* n);

/* approximate_read_overlap (:491-507) on the CURRENT component lists, for n id pairs (x[i], y[i]).  S is
 * the set of KmerIDs present in both ids' current lists (a survivor's union, any other id's own
 * sorted_kid slice); shared[i] = |S| counted as distinct KmerIDs; overlap[i] = 0 if S is empty, else the
 * larger of max - min over S of read_metas[x].kmer_positions and of read_metas[y].kmer_positions, each
 * id's OWN read, a KmerID the read does not hold reading as 0 (operator[] default; only a union can
 * contain one).  x[i] == y[i] is allowed; an id without hits gives 0 / 0.  overlap, shared: n entries
 * each, either may be NULL.  An id outside the lookup's reads: HGA_ERR_INVALID with nothing launched.
 * n == 0 is HGA_OK.  Before any merge, and after hga_components_reset, equal to hga_read_overlaps.
 * Synchronous; writes neither the component state nor the lookup's arrays. */
hga_status hga_components_overlaps(hga_ctx* ctx, const uint32_t* x, const uint32_t* y, uint64_t n,
                                   int32_t* overlap /* n, may be NULL */, uint32_t* shared /* n, may be NULL */);

/* accumulate_kmer_ids (:341-347) of id groups and the sizes of their pairwise intersections (:621-624).
 * Set s is ids[set_ptr[s] .. set_ptr[s+1]); U_s is the distinct union of its members' current lists (a
 * member listed twice or without hits changes nothing; an empty set gives an empty U_s).
 * set_size[s] = |U_s|; score[p] = |U_pair_a[p] & U_pair_b[p]| (a == b gives |U_a|).
 * HGA_ERR_INVALID, with nothing launched: an id outside the lookup's reads, a pair index >= n_sets, a
 * decreasing set_ptr.  n_sets == 0 or n_pairs == 0 is HGA_OK; with n_pairs == 0 the sizes are still
 * returned.  The sets are bitmap rows within a byte budget (HGA_SETS_BYTES in the environment, read at
 * call time, overrides it); beyond it the call runs over KmerID tiles.  Synchronous; writes neither the
 * component state nor the lookup's arrays. */
hga_status hga_components_set_scores(hga_ctx* ctx, const uint64_t* set_ptr, const uint32_t* ids, uint64_t n_sets,
                                     const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                                     uint64_t* score /* n_pairs */, uint64_t* set_size /* n_sets, may be NULL */);

/* ------------------------------------------------------------------------------
 * Spanning-tree tails — ReadClusteringEngine::get_spanning_tree_tails
 * (src/clustering/ReadClusteringEngine.cpp:509-573) for every scaffold tree in one call, under the
 * fixed orders of host/clustering.h ("Determinism").
 * Tree t is the edges [tree_ptr[t], tree_ptr[t+1]) of (ex, ey), in either orientation and any order.
 * Distances (uint64, modulo 2^64 as at :529): dist(start) = length(start), dist(child) = dist(parent) +
 * length(child) - overlap(parent, child); wrapped values take part in the maxima and thresholds as the
 * unsigned numbers they are.  Per tree: the first pass starts at the tree's smallest id; "farthest" is the
 * largest distance, ties to the smallest id; right = the ids with dist + tail_length > max in the pass
 * started at the first pass's farthest vertex, left = the same in the pass started at that pass's
 * farthest vertex (the right end); both ascending.  A tree without edges gives two empty lists.
 * ------------------------------------------------------------------------------ */

/* The two vertices :567-568 prints, with their distances: the farthest vertex of the second pass (right)
 * and of the third (left); all 0 for a tree without edges. */
typedef struct hga_tree_ends {
    uint32_t right_id;
    uint64_t right_dist;
    uint32_t left_id;
    uint64_t left_dist;
} hga_tree_ends;

/* overlap: one value per edge, sign-extended to 64 bits as (uint64_t)(int64_t) does (negative values are
 *   legal), or NULL: hga_components_overlaps of every edge on the current component state, computed on
 *   the device and never copied to the host.
 * read_length: per read of the current lookup result (by id - first_read_id, n_reads entries), or NULL:
 *   the lengths of the ctx's own read set; on a gathered ctx of more than one rank (hga_lookup_gather)
 *   NULL is HGA_ERR_STATE, the other ranks' reads are not there.
 * left_ptr, right_ptr: n_trees + 1 entries; left, right: caller-allocated, tree_ptr[n_trees] + n_trees
 *   entries; ends: n_trees entries, may be NULL.
 * HGA_ERR_INVALID, with the outputs untouched and no state written: a decreasing tree_ptr, an id outside
 *   the lookup's reads, an id that occurs in two trees, a "tree" that is not one (self-loop, repeated edge
 *   in either orientation, cycle, more than one connected part).  n_trees == 0 is HGA_OK.
 * Synchronous; HGA_ERR_STATE before hga_lookup_run; writes neither the component state nor the lookup's
 * arrays. */
hga_status hga_tree_tails(hga_ctx* ctx, const uint64_t* tree_ptr, const uint32_t* ex, const uint32_t* ey, uint64_t n_trees,
                          const int32_t* overlap /* tree_ptr[n_trees] entries, or NULL */,
                          const uint32_t* read_length /* n_reads, or NULL */, uint64_t tail_length,
                          uint64_t* left_ptr, uint32_t* left, uint64_t* right_ptr, uint32_t* right,
                          hga_tree_ends* ends /* n_trees, may be NULL */);

typedef struct hga_components_sizes {
    uint64_t index_entries;   /* entries of the current kmer_component_index                     */
    uint64_t survivors;       /* ids whose list is a union (survived a merge of two or more)     */
    uint64_t survivor_kmers;  /* the summed length of their current lists                        */
    uint64_t merges;          /* lists of two or more merged so far                              */
} hga_components_sizes;
hga_status hga_components_get_sizes(hga_ctx* ctx, hga_components_sizes* out);

/* The current kmer_component_index (:389-414 applied so far) as a CSR of ReadIDs: ptr[K+1],
 * ids[index_entries]; either may be NULL. */
hga_status hga_components_fetch_index(hga_ctx* ctx, uint64_t* ptr, uint32_t* ids);
/* The current KmerID list of one id (ReadComponent::discriminative_kmer_ids, :376): *n is always
 * set; kmers (may be NULL) receives *n entries. */
hga_status hga_components_fetch_kmers(hga_ctx* ctx, uint32_t id, uint32_t* kmers, uint64_t* n);
/* Back to the lookup's state (what construct_indices leaves, :234-299). */
hga_status hga_components_reset(hga_ctx* ctx);

/* ------------------------------------------------------------------------------
 * Spanning forest — the connections union_find accepts
 * (src/clustering/ReadClusteringEngine.cpp:424-489) when it has no rejection rule beyond "same
 * component": max_component_size = -1 and no restricted id, the first call of run_clustering in the
 * default configuration (:754-761).  The loop is Kruskal's over the list in order, so with an edge's
 * weight its position in the list (all distinct) the accepted edges are the unique minimum spanning
 * forest of the multigraph, and the device finds them in parallel (Boruvka rounds).
 * Replaying union_find over the accepted edges alone, in position order, gives the merge sequence
 * of the full list: every other connection found get_parent(x) == get_parent(y) and changed
 * nothing.  So the ComponentList member order (merge_components keeps the first member, :366), the
 * SpanningTree edge order and the order of the result are the same, and a caller fetches at most
 * n_reads - 1 edges instead of the list.  (An id that occurs in self-loops only is in no accepted
 * edge, so the replay does not return its one-member component; get_connections lists no
 * self-loop, :316.)
 * Restricted ids (hga_spanning_forest_restricted): with max_component_size = -1 the loop also
 * rejects a connection whose two components both hold a restricted id (:456; the flag of a merged
 * component is the OR of its parts, :478).  That is still a spanning forest: contract all
 * restricted ids into one vertex R.  By induction over the list the components of the contracted
 * graph are the original ones with all restricted-holding components fused into R's.  A
 * connection inside one original component is inside one contracted component; a connection
 * between two restricted-holding components is inside R's component; any other connection joins
 * two distinct components in both graphs, and accepting it merges the corresponding components
 * in both.  So the accepted positions are those of the plain loop on the contracted multigraph,
 * its unique minimum spanning forest with the position as weight, and the device runs the same
 * rounds from a start in which every restricted id already points at R.  A connection between
 * two restricted ids is a self-loop there and is never accepted.  The replay carries over
 * unchanged: union_find(accepted connections, restricted, min, -1) repeats the merges of the
 * full list, every other connection having changed nothing.  What the replay does not return is
 * again the one-member component of an id with no accepted connection, now also a restricted id
 * that only ever meets restricted-holding components; the enrichment step, the one restricted
 * call of run_clustering (:788-789), asks for components of at least 2.
 * Only a size-capped call (max_component_size != -1) is not answered: whether it rejects a
 * connection depends on component sizes, so its accepted sets are not the independent sets of
 * a matroid and the order of finding them matters.
 * ------------------------------------------------------------------------------ */

/* Edges: x == NULL and y == NULL: the ctx's current ordered connection result, i.e. what
 *   hga_connections_fetch_range returns (after hga_connections_run, hga_components_connections or
 *   hga_connections_gather; n is ignored; HGA_ERR_STATE without one).  Both given: n host pairs of
 *   ReadIDs, copied.  Exactly one NULL: HGA_ERR_INVALID.  The call works on entries
 *   [first, first + count), clipped to the list as hga_connections_fetch_range clips; more than
 *   2^32 - 2 entries after clipping: HGA_ERR_INVALID (positions are 32-bit on the device).
 * Vertices: the ReadIDs of the current lookup result, [first_read_id, first_read_id + n_reads) (the
 *   whole input's after hga_lookup_gather).  A given id outside them: HGA_ERR_INVALID with nothing
 *   launched.  x[i] == y[i] is legal and never accepted.
 * Result: the positions p, ascending and absolute (first + the place in the range), at which the
 *   reference loop finds get_parent(x) != get_parent(y); *n_edges (must not be NULL) = their number,
 *   0 for an empty range.
 * Synchronous; HGA_ERR_STATE before hga_lookup_run.  The connection result is only read. */
hga_status hga_spanning_forest(hga_ctx* ctx, const uint32_t* x, const uint32_t* y, uint64_t n, uint64_t first,
                               uint64_t count, uint64_t* n_edges);
/* hga_spanning_forest with restricted ids.  Edges, range, clipping, vertices, state rules and
 * synchrony as there; the result is fetched with hga_spanning_forest_fetch.
 * restricted: n_restricted ReadIDs in host memory, copied; duplicates, ids that occur in no edge
 *   and ids without hits are legal.  An id outside the lookup's reads: HGA_ERR_INVALID with nothing
 *   launched.  NULL with n_restricted > 0: HGA_ERR_INVALID.  n_restricted == 0: the call is
 *   hga_spanning_forest (restricted is not read).
 * Result: the positions p, ascending and absolute, at which the reference loop finds two different
 *   parents that do not both hold a restricted id.
 * A failed call leaves no result: hga_spanning_forest_fetch returns HGA_ERR_STATE until the next
 * call that succeeds. */
hga_status hga_spanning_forest_restricted(hga_ctx* ctx, const uint32_t* x, const uint32_t* y, uint64_t n,
                                          uint64_t first, uint64_t count, const uint32_t* restricted,
                                          uint64_t n_restricted, uint64_t* n_edges);
/* Copies the last result (caller-allocated, n_edges entries each; any may be NULL): the positions
 * and the connections' x and y at them.  Valid until the next hga_spanning_forest[_restricted] or
 * hga_lookup_run; HGA_ERR_STATE before any. */
hga_status hga_spanning_forest_fetch(hga_ctx* ctx, uint64_t* pos, uint32_t* x, uint32_t* y);

/* ------------------------------------------------------------------------------
 * Measurement: per-kernel device time, recorded with HIP events on the ctx stream.
 * ------------------------------------------------------------------------------ */
hga_status hga_profile_enable(hga_ctx* ctx, int on);
/* Restricts event timing to the comma-separated launch names ("" or NULL = all), so that
 * the untimed launches carry no event overhead. */
hga_status hga_profile_select(hga_ctx* ctx, const char* names);
hga_status hga_profile_reset(hga_ctx* ctx);
/* Total milliseconds and launch count recorded for kernel `name` since the reset. */
hga_status hga_profile_get(hga_ctx* ctx, const char* name, double* ms, uint64_t* launches);
/* Blocks until the ctx stream is idle. */
hga_status hga_sync(hga_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* HGA_H */
