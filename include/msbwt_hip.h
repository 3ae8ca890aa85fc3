/*
 * msbwt_hip.h -- C ABI of the MI355X (gfx950) implementation of rust-msbwt's RleBWT
 * count_kmer / constrain_range path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  Each
 * entry point names the reference interface it replaces (file:line relative to the
 * reference repo root).  The Rust side a maintainer would add -- `impl BWT for GpuRleBWT`
 * over these symbols -- is shown in INTEGRATION.md.
 *
 * Every query entry point runs on the GPU.  There is no CPU fallback: when no HIP device
 * is usable the calls return MSBWT_ERR_HIP.
 *
 * Threading: query calls on a loaded handle may be made from several host threads (they
 * serialise on the handle's stream); load calls need exclusive access, like `&mut self`
 * in the reference.
 */
#ifndef MSBWT_HIP_H
#define MSBWT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* src/msbwt_core.rs:3-14 */
#define MSBWT_VC_LEN 6      /* $ A C G N T */
#define MSBWT_LETTER_BITS 3
#define MSBWT_NUMBER_BITS 5
#define MSBWT_NUM_POWER 32
#define MSBWT_MASK 0x07
#define MSBWT_COUNT_MASK 0x1F

/* Return codes.  The reference reports file problems as io::Error and panics on malformed
 * headers / symbols >= 6; nothing unwinds across this ABI, so both become codes that the
 * Rust shim maps back. */
#define MSBWT_OK 0
#define MSBWT_ERR_IO (-1)              /* io::Error from open/metadata/read            */
#define MSBWT_ERR_UNEXPECTED_EOF (-2)  /* io::ErrorKind::UnexpectedEof (size mismatch) */
#define MSBWT_ERR_BAD_HEADER (-3)      /* reference panics (rle_bwt.rs:91-93,115,123-125) */
#define MSBWT_ERR_INVALID_SYMBOL (-4)  /* reference panics (msbwt_core.rs:127, rle_bwt.rs:212) */
#define MSBWT_ERR_INVALID_RANGE (-5)   /* l > h or h > total (reference: OOB panic / underflow) */
#define MSBWT_ERR_HIP (-6)             /* HIP runtime error or no usable device         */
#define MSBWT_ERR_NOT_LOADED (-7)
#define MSBWT_ERR_TOO_LARGE (-8)       /* total symbols >= 2^40 (device block counts are 40-bit) */
#define MSBWT_ERR_INVALID_ARG (-9)
#define MSBWT_ERR_INTERNAL (-10)       /* a device-side consistency check failed (a bug, not bad input) */
#define MSBWT_ERR_OVERFLOW (-11)       /* a count did not fit the wire width of msbwt_rle_allgather_counts */
#define MSBWT_ERR_RCCL (-12)           /* RCCL missing (librccl.so is bound at run time) or an RCCL call failed */

typedef struct msbwt_rle msbwt_rle; /* opaque; replaces `struct RleBWT` (src/rle_bwt.rs:14-24) */

/* RleBWT::with_bin_power (src/rle_bwt.rs:309-322); RleBWT::new() == bin_power 8 (:297).
 * bin_power is accepted for interface compatibility; results never depend on it (the
 * device index always uses its own fixed block size).  `device` is the HIP ordinal, -1 =
 * the current device.  Returns NULL when out of memory. */
msbwt_rle *msbwt_rle_new(uint8_t bin_power);
msbwt_rle *msbwt_rle_new_on_device(uint8_t bin_power, int device);
void msbwt_rle_free(msbwt_rle *bwt);

/* BWT::load_vector (src/msbwt_core.rs:43, src/rle_bwt.rs:59-66).  Copies: the caller keeps
 * (or drops) its Vec<u8>.  The bytes are uploaded and expanded into the query layout on the
 * device (what calculate_totals + construct_fmindex, src/rle_bwt.rs:352-467, do on the CPU);
 * MSBWT_BUILD=host in the environment selects the host-side builder instead. */
int msbwt_rle_load_vector(msbwt_rle *bwt, const uint8_t *rle_bytes, size_t len);
/* BWT::load_numpy_file (src/msbwt_core.rs:58, src/rle_bwt.rs:81-155). */
int msbwt_rle_load_numpy_file(msbwt_rle *bwt, const char *utf8_path);
/* BWT::get_symbol_count (src/msbwt_core.rs:75, src/rle_bwt.rs:172-175); 0 if symbol >= 6 */
uint64_t msbwt_rle_get_symbol_count(const msbwt_rle *bwt, uint8_t symbol);
/* BWT::get_total_size (src/msbwt_core.rs:90, src/rle_bwt.rs:190-193) */
uint64_t msbwt_rle_get_total_size(const msbwt_rle *bwt);
/* BWT::constrain_range (src/msbwt_core.rs:99, src/rle_bwt.rs:202-287).  BWTRange is not
 * repr(C), so l/h travel as scalars. */
int msbwt_rle_constrain_range(const msbwt_rle *bwt, uint8_t sym, uint64_t l, uint64_t h,
                              uint64_t *out_l, uint64_t *out_h);
/* BWT::count_kmer (src/msbwt_core.rs:124-161).  kmer: k symbol codes 0..5. */
int msbwt_rle_count_kmer(const msbwt_rle *bwt, const uint8_t *kmer, size_t k, uint64_t *out_count);

/* ---- batch extensions: the GPU entry points proper (the reference has no batch API; each
 * element is exactly one count_kmer / constrain_range call) ---- */
/* kmers: n x k row-major, one byte per symbol (codes 0..5); out_counts: n.  Host pointers. */
int msbwt_rle_count_kmers(const msbwt_rle *bwt, const uint8_t *kmers, size_t k, size_t n,
                          uint64_t *out_counts);
int msbwt_rle_constrain_ranges(const msbwt_rle *bwt, const uint8_t *syms, const uint64_t *l,
                               const uint64_t *h, size_t n, uint64_t *out_l, uint64_t *out_h);
/* Same, with DEVICE pointers on the handle's device; asynchronous on `hip_stream` (a
 * hipStream_t, NULL = default stream).  Invalid input is reported by
 * msbwt_rle_device_status(), which synchronises the stream (the device entry points keep their
 * own status word: a host-pointer call on another thread never sees or clears it).
 * Alignment: d_kmers should be 16-byte aligned -- then 1 <= k <= 64 runs the fast kernels; an
 * unaligned batch is still counted correctly, by the slower generic kernel.
 * Streams: launches queued on ONE stream share a block of tile-ticket counters (the stream orders them); launches on different
 * streams -- and on hipStreamPerThread, whose one handle value stands for a different queue in every host thread -- get blocks of
 * their own, handed back when the launch that used them has completed. */
int msbwt_rle_count_kmers_device(const msbwt_rle *bwt, const void *d_kmers, size_t k, size_t n,
                                 void *d_out_counts, void *hip_stream);
int msbwt_rle_constrain_ranges_device(const msbwt_rle *bwt, const void *d_syms, const void *d_l,
                                      const void *d_h, size_t n, void *d_out_l, void *d_out_h,
                                      void *hip_stream);
int msbwt_rle_device_status(const msbwt_rle *bwt, void *hip_stream);

/* ---- k-mer ranges and left-extension counts (no reference counterpart: the trait keeps the range inside count_kmer,
 * src/msbwt_core.rs:124-161) ----
 * Queries as for msbwt_rle_count_kmers: n x k row-major symbol codes ($ A C G N T = 0..5), any k including 0.
 * Error codes, the device forms' asynchrony (msbwt_rle_device_status), unaligned d_kmers and the host forms' pinned pipeline are
 * those of msbwt_rle_count_kmers[_device]; a row holding a code >= 6 comes back all-ones (MSBWT_ERR_INVALID_SYMBOL), every other
 * row stays exact.  Results never depend on a knob (MSBWT_* or msbwt_rle_set_*), and batch ordering (MSBWT_ORDER,
 * msbwt_rle_set_batch_order) does not apply to these calls: they always search in the caller's order.
 *
 * FM range of each k-mer: [l, h) after constrain_range on every symbol, last first, from [0, total)
 * (src/msbwt_core.rs:128-160).  h - l == count_kmer(row).  A row whose count is 0 gets l = h = 0.  k = 0: [0, total).
 * With msbwt_rle_constrain_ranges a caller can carry a search on one symbol at a time instead of searching a longer k-mer anew. */
int msbwt_rle_kmer_ranges(const msbwt_rle *bwt, const uint8_t *kmers, size_t k, size_t n,
                          uint64_t *out_l, uint64_t *out_h);
int msbwt_rle_kmer_ranges_device(const msbwt_rle *bwt, const void *d_kmers, size_t k, size_t n,
                                 void *d_out_l, void *d_out_h, void *hip_stream);

/* Left-extension counts: out[6*i + c] = count_kmer([c] ++ row i) for c = 0..5 ($ A C G N T).
 * The six sum to count_kmer(row i).  k = 0: the six symbol counts.  One search plus the index line(s) of the range's two bounds,
 * instead of six searches of k + 1 symbols.
 * Right extensions: on an index that holds every read AND its reverse complement, count(q . c) = count(rc(c . rc(q))), so
 *     count(q . c) = ext(rc(q))[COMPLEMENT_INT[c]]    (reverse_complement_i / COMPLEMENT_INT, src/string_util.rs:12,45-50)
 * -- the right extensions of q are the left extensions of rc(q), one call.  On a single-strand index right extensions are
 * separate searches of the (k+1)-mers q . c (msbwt_rle_count_kmers). */
int msbwt_rle_count_kmer_extensions(const msbwt_rle *bwt, const uint8_t *kmers, size_t k, size_t n,
                                    uint64_t *out_counts /* n x 6 */);
int msbwt_rle_count_kmer_extensions_device(const msbwt_rle *bwt, const void *d_kmers, size_t k, size_t n,
                                           void *d_out_counts /* n x 6 u64 */, void *hip_stream);

/* ---- compact queries: two bits per symbol (no reference counterpart; the trait's count_kmer takes one byte per symbol,
 * src/msbwt_core.rs:125, codes as string_util.rs:15-67 makes them) ----
 * A k-mer over ACGT, 1 <= k <= 64, as ceil(k / 32) u64 words: the k-mer read as a base-4 number with A C G T -> 0 1 2 3 and
 * its FIRST symbol most significant -- the usual 2-bit k-mer of k-mer counters: the last symbol sits in bits 0-1 of word 0,
 * symbol k-33 (k > 32) in bits 0-1 of word 1; bits beyond 2k are ignored.  8 bytes per 31-mer instead of 31: the host entry
 * point moves 8 + 8 (or 8 + 4) bytes per query over PCIe instead of 31 + 8, and the search kernel reads the words as they are.
 * '$' and 'N' cannot be said: such queries go through msbwt_rle_count_kmers.  Counts are those of the byte form, always.
 * msbwt_kmers_pack_2bit: n x k symbol codes -> words (MSBWT_ERR_INVALID_SYMBOL for a code outside A C G T).
 * count_bits: 64 (uint64_t out_counts[n]) or 32 (uint32_t out_counts[n]; a count that does not fit makes the call return
 * MSBWT_ERR_OVERFLOW).  Device form: d_kmers2bit 8-byte aligned, u64 counts, asynchronous like msbwt_rle_count_kmers_device. */
int msbwt_kmers_pack_2bit(const uint8_t *kmers, size_t k, size_t n, uint64_t *out_words);
int msbwt_rle_count_kmers_packed(const msbwt_rle *bwt, const uint64_t *kmers2bit, size_t k, size_t n, void *out_counts, int count_bits);
int msbwt_rle_count_kmers_packed_device(const msbwt_rle *bwt, const void *d_kmers2bit, size_t k, size_t n, void *d_out_counts, void *hip_stream);

/* Fused query preparation + counting: every k-mer window of every read, on the forward strand
 * and/or reverse-complemented, without materialising the n x k query matrix.  Replaces the
 * host-side loop  convert_stoi (src/string_util.rs:63-67) -> windows -> reverse_complement_i
 * (:45-50) -> count_kmer (src/msbwt_core.rs:124-161)  that consumers of the crate write.
 * reads: n_reads x read_len bytes, ASCII (ascii != 0: A/a C/c G/g T/t $ as in
 * string_util.rs:15-32, everything else N) or symbol codes (ascii == 0).  1 <= k <= 64,
 * k <= read_len.  out_fwd / out_rc: n_reads x (read_len - k + 1) counts; either may be NULL.
 * out_rc[r][w] is the count of reverse_complement_i(window w of read r). */
int msbwt_rle_count_read_kmers(const msbwt_rle *bwt, const uint8_t *reads, size_t read_len, size_t n_reads,
                               size_t k, int ascii, uint64_t *out_fwd, uint64_t *out_rc);
int msbwt_rle_count_read_kmers_device(const msbwt_rle *bwt, const void *d_reads, size_t read_len, size_t n_reads,
                                      size_t k, int ascii, void *d_out_fwd, void *d_out_rc, void *hip_stream);
/* The same for reads of different lengths (host pointers): read r is
 * reads[read_offsets[r] .. read_offsets[r+1]).  Counts are written window-major in read order:
 * read r owns out[W_r .. W_r + max(0, len_r - k + 1)) with W_r the running sum over earlier
 * reads; *out_windows (optional) receives the total.  out arrays must hold that many u64 --
 * call with out_fwd == out_rc == NULL to obtain the total only. */
int msbwt_rle_count_ragged_read_kmers(const msbwt_rle *bwt, const uint8_t *reads, const uint64_t *read_offsets,
                                      size_t n_reads, size_t k, int ascii, uint64_t *out_fwd, uint64_t *out_rc,
                                      uint64_t *out_windows);

/* ---- construction: the multi-string BWT of a read set, built on the device ----
 * DynamicBWT::create_from_fastx (src/dynamic_bwt.rs:453-473) with the semantics of naive_bwt (src/bwt_util.rs:154-171): the
 * text is every read followed by '$', its suffixes sorted with $ < A < C < G < N < T, suffixes that are equal up to and
 * including their '$' ordered by the rank of their reads; row i is the symbol before suffix i.  The entry points use the
 * handle's device, stream, mutex and msbwt_rle_last_error; the handle need not hold an index.
 *
 * reads: read r is reads[read_offsets[r] .. read_offsets[r+1]); ascii != 0: bytes as string_util.rs:15-32 maps them
 * (A/a C/c G/g T/t, anything else N; '$' is an error), ascii == 0: symbol codes 1..5.
 * out_rle/cap: caller's buffer; read_offsets[n_reads] + n_reads bytes always suffice.  *out_len: bytes written -- or,
 * with MSBWT_ERR_INVALID_ARG and nothing written, the bytes needed when cap is too small.
 * Checked on the host before anything is launched: null pointers with n_reads > 0 or decreasing offsets
 * (MSBWT_ERR_INVALID_ARG), 2^40 symbols or more (MSBWT_ERR_TOO_LARGE), a code 0 or >= 6 / a '$' (MSBWT_ERR_INVALID_SYMBOL).
 * n_reads == 0 is the empty BWT.  A piece that does not fit HBM: MSBWT_ERR_HIP, the message names the piece size. */
int msbwt_rle_build_from_reads(msbwt_rle *bwt, const uint8_t *reads, const uint64_t *read_offsets, size_t n_reads,
                               int ascii, uint8_t *out_rle, size_t cap, uint64_t *out_len);
/* The same build, then the result loaded exactly as msbwt_rle_load_vector would load those bytes (an index the handle
 * holds is released before the build: its HBM is the builder's to use). */
int msbwt_rle_load_reads(msbwt_rle *bwt, const uint8_t *reads, const uint64_t *read_offsets, size_t n_reads, int ascii);
/* Most suffixes sorted at once (0 = automatic, from the free HBM); env MSBWT_BUILD_PIECE.  Results never depend on it. */
int msbwt_rle_set_build_piece(msbwt_rle *bwt, uint64_t suffixes);
/* Pure function, no device: HBM bytes the build of `total_symbols` symbols needs with pieces of `piece` suffixes
 * (0 = the automatic piece), and the automatic piece for `free_hbm_bytes`.  Either output may be NULL. */
int msbwt_build_reads_plan(uint64_t total_symbols, uint64_t free_hbm_bytes, uint64_t piece, uint64_t *auto_piece,
                           uint64_t *device_bytes);
/* Suffixes one workgroup ranks and scatters per radix pass of the builder (tests probe its borders). */
size_t msbwt_build_reads_sort_tile(void);
/* Milliseconds the stages of the handle's last build took (host clock, the stream drained at every stage border):
 * copy in, read order, histogram, collect, sort, emit, encode, copy out; *out_pieces (optional): pieces sorted. */
#define MSBWT_BUILD_STAGES 8
int msbwt_rle_build_stage_ms(const msbwt_rle *bwt, double *out_ms, uint64_t *out_pieces);

/* ---- merge: two multi-string BWTs -> the BWT of the union of their read sets, on the device ----
 * bwt_util::pairwise_bwt_merge (src/bwt_util.rs:21-141), the interleave iteration of Holt & McMillan 2014: no reads and no
 * suffix sort, the two symbol arrays and a bit per merged row.  The entry points use the handle's device, stream, mutex and
 * msbwt_rle_last_error; the handle need not hold an index.
 *
 * rle0 / rle1: RLE bytes as msbwt_rle_load_vector takes them; a run may span any number of bytes and hold zero digits, the
 * encoding need not be the canonical one.  Either may be empty (len 0, the pointer may be NULL); two empty inputs give the
 * empty BWT without touching the device.
 * out_rle/cap: caller's buffer, the canonical encoding (what convert_to_vec gives); len0 + len1 bytes always suffice for
 * canonical inputs.  *out_len: bytes written -- or, with MSBWT_ERR_INVALID_ARG and nothing written, the bytes needed when cap
 * is too small.
 * out_from_second (optional): ceil(total / 8) bytes; bit i & 7 of byte i >> 3 is set when merged row i came from rle1.  Rows
 * of equal rotations: those of rle0 first.
 * Checked on the host before anything is launched: a null input with a length, a null out_len (MSBWT_ERR_INVALID_ARG), a
 * symbol code >= 6 (MSBWT_ERR_INVALID_SYMBOL), a merged total of 2^40 symbols or more (MSBWT_ERR_TOO_LARGE).  HBM that does
 * not suffice: MSBWT_ERR_HIP, the message names the bytes needed (msbwt_merge_plan). */
int msbwt_rle_merge(msbwt_rle *bwt, const uint8_t *rle0, size_t len0, const uint8_t *rle1, size_t len1,
                    uint8_t *out_rle, size_t cap, uint64_t *out_len, uint8_t *out_from_second);
/* The same merge, then the result loaded exactly as msbwt_rle_load_vector would load those bytes (an index the handle
 * holds is released before the merge: its HBM is the merge's to use). */
int msbwt_rle_load_merged(msbwt_rle *bwt, const uint8_t *rle0, size_t len0, const uint8_t *rle1, size_t len1);
/* Pure function, no device: HBM bytes the merge of BWTs of total0 and total1 symbols needs, at most
 * 2.5 x (total0 + total1) + 64 MiB.  MSBWT_ERR_TOO_LARGE from 2^40 merged symbols on. */
int msbwt_merge_plan(uint64_t total0, uint64_t total1, uint64_t *device_bytes);
/* ---- merge of any number of BWTs in one pass ----
 * The same iteration over a byte per merged row, the index of the input the row came from, in place of a bit: one round whatever
 * the number of inputs, where a tree of msbwt_rle_merge calls takes ceil(log2 n) rounds over every symbol.
 *
 * Input i is rle[rle_offsets[i] .. rle_offsets[i + 1]) (n_inputs + 1 offsets, as msbwt_rle_build_from_reads takes reads): RLE
 * bytes as msbwt_rle_load_vector takes them; a run may span any number of bytes and hold zero digits; any input may be empty.
 * out_rle, cap and out_len: as msbwt_rle_merge; the bytes are what a left fold of msbwt_rle_merge over the inputs gives.
 * out_source (optional): one byte per merged row, the index of the input the row came from.  Rows of equal rotations: lower
 * input index first, and within one input its own order.  With two inputs it is msbwt_rle_merge's bit vector written as bytes.
 * One input is re-encoded canonically; no input, or only empty ones, give the empty BWT and nothing touches the device.
 * Checked on the host before anything is launched: more than MSBWT_MERGE_MAX_INPUTS inputs, a null pointer where a length is
 * given, decreasing offsets, a null out_len (MSBWT_ERR_INVALID_ARG), a symbol code >= 6 (MSBWT_ERR_INVALID_SYMBOL, the message
 * names the input), a merged total of 2^40 symbols or more (MSBWT_ERR_TOO_LARGE).  HBM that does not suffice: MSBWT_ERR_HIP,
 * the message names the bytes needed (msbwt_merge_many_plan).  msbwt_rle_merge_info reports the handle's last merge of either
 * kind. */
#define MSBWT_MERGE_MAX_INPUTS 32
int msbwt_rle_merge_many(msbwt_rle *bwt, const uint8_t *rle, const uint64_t *rle_offsets, size_t n_inputs,
                         uint8_t *out_rle, size_t cap, uint64_t *out_len, uint8_t *out_source);
/* The same merge, then the result loaded exactly as msbwt_rle_load_vector would load those bytes (an index the handle
 * holds is released before the merge: its HBM is the merge's to use). */
int msbwt_rle_load_merged_many(msbwt_rle *bwt, const uint8_t *rle, const uint64_t *rle_offsets, size_t n_inputs);
/* Pure function, no device: HBM bytes the one-pass merge of n_inputs BWTs of totals[i] symbols needs: with T their sum, at
 * least 2 x T and at most 3.25 x T + 64 MiB (a byte per symbol for the decoded inputs, two source arrays of a byte per row,
 * n_inputs + 6 counts per tile).  It depends on the totals through their sum alone.  MSBWT_ERR_INVALID_ARG beyond
 * MSBWT_MERGE_MAX_INPUTS inputs, MSBWT_ERR_TOO_LARGE from 2^40 merged symbols on. */
int msbwt_merge_many_plan(const uint64_t *totals, size_t n_inputs, uint64_t *device_bytes);
/* Merged rows one workgroup counts and scatters per iteration (tests probe its borders). */
size_t msbwt_merge_tile(void);
/* The handle's last merge, of two inputs or of many: its iterations (the last one found nothing to change) and the milliseconds of its stages (host
 * clock, the stream drained at every stage border): copy in, decode, iterate, emit, encode, copy out.  Either may be NULL. */
#define MSBWT_MERGE_STAGES 6
int msbwt_rle_merge_info(const msbwt_rle *bwt, uint64_t *iterations, double *out_ms);

/* ---- counts by source: how often a k-mer occurs in each input of a merged BWT (no reference counterpart) ----
 * The rows of input i inside the merged range of a k-mer are exactly the occurrences of the k-mer in input i.  So with the merge's
 * source vector attached to the loaded index, one search gives a k-mer's count in every input: column i of a result equals
 * count_kmer on input i's own BWT, and the columns sum to count_kmer on the merged one.
 *
 * msbwt_rle_set_sources: attaches `sources`, a host array of one byte per row -- exactly what out_source of msbwt_rle_merge_many
 * holds -- to the loaded index: the vector goes to HBM (in pieces through the pinned staging of the host batches) with one checkpoint
 * of counts per msbwt_source_block_rows rows.  Checked on the host: an index is loaded (MSBWT_ERR_NOT_LOADED), n_rows equals
 * msbwt_rle_get_total_size and 1 <= n_sources <= MSBWT_MERGE_MAX_INPUTS (MSBWT_ERR_INVALID_ARG); on the device, while the checkpoints
 * are built: every byte < n_sources (MSBWT_ERR_INVALID_ARG).  Whatever was attached before is gone once the call has found an index,
 * however it ends.  sources == NULL with n_sources == 0 detaches.  HBM that does not suffice: MSBWT_ERR_HIP, the message names the
 * bytes needed (msbwt_source_index_plan).
 * Lifetime: every load (msbwt_rle_load_vector, _load_numpy_file, _load_reads, _load_merged*) drops the attachment; the setters that
 * rebuild optional structures (msbwt_rle_set_sparse_table, msbwt_rle_set_query_length, ...) keep it, the rows do not move;
 * msbwt_rle_replicate copies it; msbwt_rle_device_bytes includes it.  It is the caller's explicit request and does NOT count
 * against the plan of msbwt_rle_set_memory_budget. */
int msbwt_rle_set_sources(msbwt_rle *bwt, const uint8_t *sources, uint64_t n_rows, size_t n_sources);
/* msbwt_rle_load_merged_many, then the merge's own source vector attached (n_inputs sources); the vector stays in HBM between the
 * two.  No inputs at all: nothing is attached. */
int msbwt_rle_load_merged_many_sources(msbwt_rle *bwt, const uint8_t *rle, const uint64_t *rle_offsets, size_t n_inputs);
/* Sources attached (0: none), and the rows of each (MSBWT_ERR_NOT_LOADED without an attachment). */
int msbwt_rle_source_count(const msbwt_rle *bwt);
int msbwt_rle_source_totals(const msbwt_rle *bwt, uint64_t *out /* n_sources */);
/* out[n_sources * i + s] = occurrences of row i in input s.  Queries, error codes, the device form's asynchrony, the all-ones row
 * of a query holding a code >= 6 and "always in the caller's order, whatever the knobs" are those of msbwt_rle_kmer_ranges[_device].
 * k = 0: the source totals.  A k-mer that does not occur: zeros.  Without sources attached: MSBWT_ERR_NOT_LOADED, the message
 * "no sources attached". */
int msbwt_rle_count_kmers_by_source(const msbwt_rle *bwt, const uint8_t *kmers, size_t k, size_t n,
                                    uint64_t *out_counts /* n x n_sources, row-major */);
int msbwt_rle_count_kmers_by_source_device(const msbwt_rle *bwt, const void *d_kmers, size_t k, size_t n,
                                           void *d_out_counts /* n x n_sources u64 */, void *hip_stream);
/* The second phase on its own, for callers who carry ranges (msbwt_rle_constrain_ranges): out[n_sources * i + s] = rows of source
 * s in [l[i], h[i]).  l == h: zeros.  l > h or h > total: an all-ones row and MSBWT_ERR_INTERNAL (the device's consistency flag, as
 * the extension counts raise it); no address is formed from such a range. */
int msbwt_rle_range_sources(const msbwt_rle *bwt, const uint64_t *l, const uint64_t *h, size_t n,
                            uint64_t *out_counts /* n x n_sources */);
int msbwt_rle_range_sources_device(const msbwt_rle *bwt, const void *d_l, const void *d_h, size_t n,
                                   void *d_out_counts /* n x n_sources u64 */, void *hip_stream);
/* Pure function, no device: HBM bytes the attachment of n_sources sources to total_rows rows holds -- the vector and the checkpoints,
 * at most 1.5 x total_rows + MSBWT_SOURCE_INDEX_SLACK at 32 sources (fewer sources: less).  MSBWT_ERR_INVALID_ARG unless
 * 1 <= n_sources <= MSBWT_MERGE_MAX_INPUTS, MSBWT_ERR_TOO_LARGE from 2^40 rows on. */
#define MSBWT_SOURCE_INDEX_SLACK 1024
int msbwt_source_index_plan(uint64_t total_rows, size_t n_sources, uint64_t *device_bytes);
/* Rows per checkpoint, a power of two; and the widest range that is counted from its own bytes without a checkpoint (tests probe
 * the borders of both). */
size_t msbwt_source_block_rows(void);
size_t msbwt_source_narrow_rows(void);

/* ---- spectrum and enumeration: the k-mers an index HOLDS, and how often (no reference counterpart) ----
 * Every other query starts from k-mers the caller brings; these start from the index.  The k-mers of an index are the strings q over
 * A C G T of length k, 1 <= k <= 32, with count_kmer(q) > 0 (a window holding '$' or 'N' is no k-mer); a k-mer's count is
 * count_kmer(q) and its range that of msbwt_rle_kmer_ranges; it is reported as ONE u64 in the packed form of msbwt_kmers_pack_2bit
 * (A C G T -> 0 1 2 3, first symbol most significant, last symbol in bits 0-1), which msbwt_rle_count_kmers_packed[_device] takes as it
 * is.  Ranges of distinct k-mers are disjoint and lie in lexicographic order: "ascending by k-mer word" and "ascending by l" are the
 * same order.  None of this depends on any knob (block format, pair index, tables, frontier).
 * How: the frontier expansion that builds the sparse table, run to depth k -- one pair-block line takes a present d-mer to all its
 * present (d+2)-mers -- from the root or from the flat direct table's non-empty entries; DESIGN.md 3, "Spectrum and enumeration".
 *
 * msbwt_rle_kmer_spectrum: out_hist[c], 1 <= c < n_bins - 1, = distinct k-mers whose count is exactly c; out_hist[n_bins - 1] = those
 * whose count is >= n_bins - 1; out_hist[0] = 0.  n_bins >= 2.  *out_distinct = the sum of the bins, *out_occurrences = the sum of all
 * counts (the ACGT-only windows of length k in the reads); either may be NULL.
 *
 * msbwt_rle_enumerate_kmers: the k-mers with min_count <= count <= max_count (max_count == 0: no upper limit; min_count == 0 is 1;
 * min_count > max_count != 0: MSBWT_ERR_INVALID_ARG) as records (k-mer, count, l); h = l + count.  *out_n is always set to the number
 * of such k-mers.  capacity == 0 (and no buffers): the call only counts -- the first half of the two-call pattern.  0 < capacity < n:
 * NOTHING is written, *out_n = n, MSBWT_ERR_INVALID_ARG and the message names n.  out_counts and out_l may each be NULL.  sorted != 0:
 * ascending k-mers, the same from run to run; sorted == 0: the order the expansion produces.  A count window prunes the walk: no k-mer
 * occurs more often than any of its suffixes, so with min_count = m a suffix narrower than m is dropped at every level (on reads with
 * errors the once-only suffixes then cost nothing).  A call that fills buffers walks twice (count, then write).
 * The _device form writes to device buffers on the handle's device and synchronises the stream (n has to reach the host); a device
 * fault is reported by msbwt_rle_device_status as elsewhere.
 *
 * Guards, before the first HIP call: NULL handle MSBWT_ERR_INVALID_ARG, nothing loaded MSBWT_ERR_NOT_LOADED ("no BWT loaded"), k
 * outside 1..32 MSBWT_ERR_INVALID_ARG.  All scratch is allocated per call and freed before it returns (msbwt_rle_device_bytes is
 * unchanged): msbwt_spectrum_plan bytes -- two frontier buffers and their cursors; sorted dumps: a bit per row and a rank checkpoint
 * per 1024 rows; host dumps: the records (24 bytes each) -- and the spectrum's 8 n_bins.  Scratch that does not fit: MSBWT_ERR_HIP,
 * the message names the bytes. */
int msbwt_rle_kmer_spectrum(const msbwt_rle *bwt, size_t k, uint64_t *out_hist, size_t n_bins,
                            uint64_t *out_distinct, uint64_t *out_occurrences);
int msbwt_rle_enumerate_kmers(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, int sorted,
                              uint64_t *out_kmers2bit, uint64_t *out_counts, uint64_t *out_l, uint64_t capacity, uint64_t *out_n);
int msbwt_rle_enumerate_kmers_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count, int sorted,
                                     void *d_out_kmers2bit, void *d_out_counts, void *d_out_l, uint64_t capacity, uint64_t *out_n,
                                     void *hip_stream);
/* Most nodes a frontier buffer of the walk holds (24 bytes each, two buffers); 0 = automatic (2^27, or what an eighth of the free HBM
 * holds, never more than rows + 1024).  The seeds are worked through in chunks that keep the frontiers inside it: a chunk that
 * overflows is taken again at half the size, a single seed whose subtree does not fit is expanded one level and its children are
 * walked in its place.  Results never depend on it; it exists so that tests reach the chunking on tiny inputs, as
 * msbwt_rle_set_build_piece does for the builder.  Below MSBWT_SPECTRUM_MIN_FRONTIER (and not 0): MSBWT_ERR_INVALID_ARG. */
#define MSBWT_SPECTRUM_MIN_FRONTIER 64
int msbwt_rle_set_spectrum_frontier(msbwt_rle *bwt, uint64_t nodes);
/* The last walk of the handle (of a dump that filled buffers: the writing walk): [0] k, [1] seed depth (0: from the root), [2] chunks
 * run, [3] chunks taken again at half size after an overflow, [4 + d], d = 0..32: nodes at depth d that survived the pruning ([4 + k]:
 * the k-mers the sink took), [37] milliseconds of the whole call (rounded), [38] the same in microseconds, [39] single seeds that were
 * expanded a level and re-seeded. */
#define MSBWT_SPECTRUM_INFO_WORDS 40
int msbwt_rle_spectrum_info(const msbwt_rle *bwt, uint64_t *out /* MSBWT_SPECTRUM_INFO_WORDS */);
/* Pure function, no device: bytes of HBM a call on an index of total_rows rows allocates with free_hbm_bytes free and the automatic
 * frontier -- `records` records staged for a host dump (0 for the _device form, for counting and for the spectrum, which adds
 * 8 n_bins).  MSBWT_ERR_TOO_LARGE from 2^40 rows (or records) on.  device_bytes may be NULL. */
int msbwt_spectrum_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t records, int sorted, uint64_t *device_bytes);

/* ---- canonical k-mers: the spectrum and the dump with a k-mer and its reverse complement as ONE k-mer (no reference counterpart) ----
 * Reads come from both strands, so a census of k-mers counts q and rc(q) together (a k-mer counter's "canonical" mode).
 * rc(q) is the reverse complement of a k-mer over A C G T (COMPLEMENT_INT, msbwt_reverse_complement_i); on the packed 2-bit form
 * (A C G T -> 0 1 2 3, first symbol most significant) it reverses the order of the k 2-bit fields and XORs each with 3.  The CANONICAL
 * k-mer of the class {q, rc(q)} is the one with the smaller packed word (lexicographic order and word order agree).  A class OCCURS
 * when count_kmer(q) + count_kmer(rc(q)) > 0 and is reported as ONE record (w, own, other): w the canonical word, own = count_kmer(w),
 * other = count_kmer(rc(w)) -- for a palindrome (w == rc(w), even k only) other = 0.  The class's COUNT is own + other, so a palindrome
 * is counted once, not twice, and the counts of all classes sum to the `occurrences` of the plain spectrum.
 *
 * msbwt_kmers_reverse_complement_2bit: pure host function, no device: out[i] = packed reverse complement of words[i] (bits above 2 k
 * are ignored); 1 <= k <= 32, else MSBWT_ERR_INVALID_ARG.  words == out is allowed.
 *
 * msbwt_rle_canonical_kmer_spectrum: as msbwt_rle_kmer_spectrum over the classes: out_hist[min(count, n_bins - 1)] += 1 per class, bin 0
 * empty, *out_distinct = the classes, *out_occurrences = the sum of their counts.
 * msbwt_rle_enumerate_canonical_kmers[_device]: the classes whose count own + other lies in the window (min_count == 0 is 1, max_count
 * == 0: no upper limit, min_count > max_count != 0: MSBWT_ERR_INVALID_ARG), with the two-call capacity pattern of
 * msbwt_rle_enumerate_kmers: capacity == 0 only counts; 0 < capacity < n writes NOTHING, sets *out_n = n, returns
 * MSBWT_ERR_INVALID_ARG and names n in the message.  out_own and out_other may each be NULL.  A call that fills buffers walks twice.
 * ORDER: the records come in the order the walk produces them, and there is no `sorted` argument -- a class whose canonical member is
 * absent from the index has no row of its own, so the placement by rank that sorts the plain dump does not carry over, and the
 * library has no general device sort.  Sort by word on the host where order matters (the Python mirror does, on request).
 *
 * How: the walk of the plain calls stages each chunk's k-mers (word, count) instead of sinking them; their reverse complements are
 * written as packed words and counted by the search behind msbwt_rle_count_kmers_packed_device; one more pass emits every class from
 * exactly one member -- the strand with the larger count, on a tie the canonical one.  With a window minimum m the walk prunes at
 * ceil(m / 2), not m: of two strands whose counts sum to m or more the larger has ceil(m / 2) or more, and so has each of its suffixes,
 * so the emitting member survives even where the other strand is pruned or absent ("Canonical spectrum").
 * Guards before the first HIP call, scratch per call and freed on return (msbwt_rle_device_bytes unchanged; what the search keeps
 * for its launches it keeps as for any count call), MSBWT_ERR_HIP naming the bytes when it does not fit, independence of every knob:
 * as for the plain calls.  msbwt_rle_spectrum_info reports the walk as it does for them: [4 + k] is the number of k-mers the last
 * level handed on (both strands, after pruning), not the number of classes. */
int msbwt_kmers_reverse_complement_2bit(const uint64_t *words, size_t k, size_t n, uint64_t *out);
int msbwt_rle_canonical_kmer_spectrum(const msbwt_rle *bwt, size_t k, uint64_t *out_hist, size_t n_bins,
                                      uint64_t *out_distinct, uint64_t *out_occurrences);
int msbwt_rle_enumerate_canonical_kmers(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count,
                                        uint64_t *out_kmers2bit, uint64_t *out_own, uint64_t *out_other, uint64_t capacity, uint64_t *out_n);
int msbwt_rle_enumerate_canonical_kmers_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t max_count,
                                               void *d_out_kmers2bit, void *d_out_own, void *d_out_other, uint64_t capacity, uint64_t *out_n,
                                               void *hip_stream);
/* Pure function, no device: bytes of HBM a canonical call allocates and frees again with the automatic frontier: what
 * msbwt_spectrum_plan(total_rows, free_hbm_bytes, 0, 0) gives for the walk -- whose last frontier IS the staging of (word, count) --
 * plus 16 bytes per frontier node for the other strand (word, count), plus 24 bytes per record staged for a host dump (0 for the
 * _device form, for counting and for the spectrum, which adds 8 n_bins).  A call's real scratch (msbwt_rle_spectrum_scratch_bytes)
 * is 256 bytes above this: the words of its totals, an allocation of their own that the plan leaves out.
 * MSBWT_ERR_TOO_LARGE from 2^40 rows (or records) on. */
int msbwt_canonical_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t records, uint64_t *device_bytes);

/* ---- k-mers by source: one spectrum per input of a merged index, and the dump filtered by per-source counts (no reference counterpart) ----
 * "The k-mers that occur at least 5 times in the tumour and never in the normal", "the k-mers all lanes share", an abundance spectrum
 * per sample out of ONE merged index: the k-mers come from the index (as in the spectrum section), their per-source counts from the
 * source vector (as msbwt_rle_range_sources), and the two meet on the device, chunk by chunk -- neither the dump of all k-mers nor an
 * n x S count matrix is ever made.  All calls need a loaded index WITH sources attached (msbwt_rle_set_sources,
 * msbwt_rle_load_merged_many_sources); S = msbwt_rle_source_count, c_s(q) = the rows of source s in q's range, which is
 * count_kmer(q) on input s's own BWT; the c_s of a k-mer sum to its count.
 *
 * msbwt_rle_kmer_spectrum_by_source: out_hist is S x n_bins, row-major; over the k-mers of the merged index out_hist[s * n_bins + c],
 * 1 <= c < n_bins - 1, = the k-mers with c_s == c, the last bin those with c_s >= n_bins - 1, and bin 0 the k-mers of the index that
 * source s does NOT hold (non-zero here, unlike in the plain spectrum).  n_bins >= 2.  out_sharing (S + 1 words, may be NULL): [j] = the
 * k-mers held by exactly j sources, [0] = 0.  out_distinct (S, may be NULL): the sum of row s's bins >= 1.  out_occurrences (S, may be
 * NULL): the sum of c_s.  Row s equals msbwt_rle_kmer_spectrum of input s loaded alone, bin 0 apart.
 *
 * msbwt_rle_enumerate_kmers_by_source[_device]: the k-mers with min_counts[s] <= c_s <= max_counts[s] for EVERY s and min_total <= sum
 * of the c_s <= max_total, as records (k-mer, c_0 .. c_{S-1}, l); out_counts is n x S, row-major.  min_counts and max_counts are HOST
 * arrays of S words in both forms; min_counts == NULL: all zeros, max_counts == NULL: no limits.
 * NOTE the convention of max_counts: UINT64_MAX means no limit and 0 means ABSENT FROM THIS SOURCE -- that is the point of the call
 * ("private to input 0": max_counts = {UINT64_MAX, 0, 0, ...}).  It deliberately differs from max_count == 0 = "no upper limit" of
 * msbwt_rle_enumerate_kmers, which min_total and max_total keep: min_total == 0 is 1, max_total == 0 is no limit.
 * min_counts[s] > max_counts[s], or min_total > max_total != 0: MSBWT_ERR_INVALID_ARG.
 * Capacity, order and the two forms are exactly msbwt_rle_enumerate_kmers': *out_n is always set; capacity == 0 only counts; 0 <
 * capacity < n writes NOTHING, sets *out_n = n, returns MSBWT_ERR_INVALID_ARG and names n in the message; out_counts and out_l may each
 * be NULL; a call that fills buffers walks twice; sorted != 0: ascending k-mers, the same from run to run (every emitted k-mer has rows
 * of its own, so the placement by the rank of l carries over); sorted == 0: the order the walk produces.  The _device form writes to
 * device buffers on the handle's device, synchronises the stream and reports a device fault through msbwt_rle_device_status.
 * The walk prunes with max(min_total, the sum of min_counts, 1): a suffix occurs at least as often as the k-mer.  (It does not prune
 * per source at inner levels.)
 *
 * Guards, before the first HIP call: NULL handle MSBWT_ERR_INVALID_ARG; nothing loaded MSBWT_ERR_NOT_LOADED ("no BWT loaded"); no
 * attachment MSBWT_ERR_NOT_LOADED ("no sources attached"); k outside 1..32 MSBWT_ERR_INVALID_ARG.  Scratch per call, freed on return
 * (msbwt_rle_device_bytes unchanged): msbwt_kmers_by_source_plan bytes, and the spectrum's 8 S n_bins.  A k-mer's S counts live in the
 * registers of the eight lanes that count it: apart from the records staged for a host dump NO scratch grows with frontier x S.
 * msbwt_rle_spectrum_info reports these walks as it does the others: [4 + k] is the number of k-mers the last level handed to the
 * sink, before the predicate ("K-mers by source"). */
int msbwt_rle_kmer_spectrum_by_source(const msbwt_rle *bwt, size_t k, uint64_t *out_hist, size_t n_bins, uint64_t *out_sharing,
                                      uint64_t *out_distinct, uint64_t *out_occurrences);
int msbwt_rle_enumerate_kmers_by_source(const msbwt_rle *bwt, size_t k, const uint64_t *min_counts, const uint64_t *max_counts,
                                        uint64_t min_total, uint64_t max_total, int sorted, uint64_t *out_kmers2bit,
                                        uint64_t *out_counts, uint64_t *out_l, uint64_t capacity, uint64_t *out_n);
int msbwt_rle_enumerate_kmers_by_source_device(const msbwt_rle *bwt, size_t k, const uint64_t *min_counts, const uint64_t *max_counts,
                                               uint64_t min_total, uint64_t max_total, int sorted, void *d_out_kmers2bit,
                                               void *d_out_counts, void *d_out_l, uint64_t capacity, uint64_t *out_n, void *hip_stream);
/* Pure function, no device: bytes of HBM a by-source call allocates and frees again with the automatic frontier: what
 * msbwt_spectrum_plan(total_rows, free_hbm_bytes, 0, sorted) gives for the walk, the sink's fixed words (its limits and totals: the
 * same at every size and every S), plus 8 (2 + n_sources) bytes per record staged for a host dump (0 for the _device form and for
 * counting).  n_sources outside 1..MSBWT_MERGE_MAX_INPUTS: MSBWT_ERR_INVALID_ARG; MSBWT_ERR_TOO_LARGE from 2^40 rows (or records) on. */
int msbwt_kmers_by_source_plan(uint64_t total_rows, uint64_t free_hbm_bytes, size_t n_sources, uint64_t records, int sorted,
                               uint64_t *device_bytes);

/* ---- the k-mer graph: how the k-mers of an index connect (no reference counterpart) ----
 * The de Bruijn graph of the reads as ONE object: the sorted k-mer dump with an edge byte per k-mer, and the table of (in, out) degrees.
 * Everything is defined through count_kmer alone.  NODES: for 1 <= k <= 32 and the node threshold m = max(min_count, 1), the k-mers q
 * over A C G T with count_kmer(q) >= m.  EDGES: with the edge threshold me (min_edge == 0: me = m; 0 < min_edge < m:
 * MSBWT_ERR_INVALID_ARG), the (k+1)-mers e over A C G T with count_kmer(e) >= me; e goes from e[0..k) to e[1..k].  Both ends of every
 * edge are nodes -- a k-mer occurs at least as often as any (k+1)-mer that holds it, and me >= m -- which is why the call has no
 * max_count: a caller drops high-copy nodes by the counts it gets back.
 * EDGE BYTE of a node q: bit j (j = 0..3 for A C G T) is set when the edge j.q exists (its predecessors), bit 4 + j when the edge q.j
 * exists (its successors).  A window that holds '$' or 'N' is no k-mer and no edge, so a read that starts or ends at q adds no bit; a
 * self-loop (A^k with A^(k+1)) sets a predecessor bit and a successor bit of the same node.
 *
 * msbwt_rle_enumerate_kmer_graph[_device]: records in ascending k-mer order, always (placement by rank is what the edge pass rests on):
 * words, counts and l exactly as msbwt_rle_enumerate_kmers(k, m, 0, sorted = 1, ..) gives them, and out_edges, one byte per record.
 * Capacity as for the other dumps: *out_n is always set; capacity == 0 only counts; 0 < capacity < n writes NOTHING, returns
 * MSBWT_ERR_INVALID_ARG and names n in the message.  Any of the four output buffers may be NULL.  The _device form writes to device
 * buffers on the handle's device (d_out_edges needs no alignment, and nothing past its first n bytes is touched), synchronises the
 * stream and reports a device fault through msbwt_rle_device_status.  A call that fills buffers walks twice (count and mark, then write).
 * msbwt_rle_kmer_graph_degrees: out_table[5 i + o] = the nodes with i predecessors and o successors; *out_nodes = the sum of the
 * table; *out_edges = the number of edges, which is the sum of the in-degrees and the sum of the out-degrees alike.  Either pointer
 * (and out_table) may be NULL.  No record leaves the device.
 *
 * How: the counting walk of the sorted dump marks every node's l; the writing walk stages each chunk's nodes, and one kernel per chunk
 * takes every node q one step to its (k+1)-mers e = c.q: each e at least me wide sets predecessor bit c of q and the successor bit
 * (last symbol of q) of e's prefix e[0..k) -- whose range holds e's, so its record is the last marked row at or below e.l (DESIGN.md
 * 3, "K-mer graph").  Results depend on no knob (block format, pair index, stride, tables, frontier).
 * Guards, before the first HIP call: NULL handle MSBWT_ERR_INVALID_ARG; nothing loaded MSBWT_ERR_NOT_LOADED ("no BWT loaded"); k
 * outside 1..32 MSBWT_ERR_INVALID_ARG; min_edge below the node threshold and not 0 MSBWT_ERR_INVALID_ARG.  Scratch per call, freed on
 * return (msbwt_rle_device_bytes unchanged); scratch that does not fit: MSBWT_ERR_HIP naming the bytes.  msbwt_rle_spectrum_info
 * reports the writing walk as it does for the others. */
int msbwt_rle_enumerate_kmer_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint64_t *out_kmers2bit,
                                   uint64_t *out_counts, uint64_t *out_l, uint8_t *out_edges, uint64_t capacity, uint64_t *out_n);
int msbwt_rle_enumerate_kmer_graph_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_kmers2bit,
                                          void *d_out_counts, void *d_out_l, void *d_out_edges, uint64_t capacity, uint64_t *out_n,
                                          void *hip_stream);
int msbwt_rle_kmer_graph_degrees(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint64_t *out_table /* 25 */,
                                 uint64_t *out_nodes, uint64_t *out_edges);
/* Pure function, no device: bytes of HBM a host dump of `records` nodes with all of words, counts and l allocates and frees again with
 * the automatic frontier, EXACTLY
 *     msbwt_spectrum_plan(total_rows, free_hbm_bytes, 0, 1)   the walk, the bit per row and the rank checkpoints
 *     + 256                                                   the 25 degree counters, padded
 *     + 4 ceil(records / 4)                                   the edge bytes: one per node, as whole 32-bit words
 *     + 24 records                                            words, counts and l staged for the host (8 records less per NULL buffer)
 * The _device form and msbwt_rle_kmer_graph_degrees stage nothing: 24 records less.  A call that only counts (capacity == 0) allocates
 * what msbwt_spectrum_plan(total_rows, free_hbm_bytes, 0, 0) says.  MSBWT_ERR_TOO_LARGE from 2^40 rows (or records) on; device_bytes
 * may be NULL. */
int msbwt_kmer_graph_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t records, uint64_t *device_bytes);

/* ---- unitigs ---- the k-mer graph compacted into its non-branching paths, on the device (no reference counterpart)
 * THE GRAPH is G(k, m, me) exactly as the section above defines it: nodes = the k-mers with count_kmer >= m = max(min_count, 1), edges =
 * the (k+1)-mers with count_kmer >= me (min_edge == 0: me = m; 0 < min_edge < m: MSBWT_ERR_INVALID_ARG), 1 <= k <= 32; in(q) = the
 * population of the low nibble of q's edge byte, out(q) that of the high nibble.
 * LINKS: an edge p -> q is a link when out(p) = 1 and in(q) = 1.  A node has at most one link in and one link out, so the links cut
 * the node set into disjoint simple paths and simple cycles; a node without links is a path of one.
 * UNITIGS: each such path or cycle is one unitig; every node belongs to exactly one.
 * CYCLES: a cycle (every edge around it a link: an isolated cycle) is opened at its smallest k-mer word: that node is the unitig's
 * first, the node whose link leads into it is its last, and the unitig is CIRCULAR.  A node whose only in-edge and only out-edge is
 * its self-loop (A^k with A^(k+1) and nothing else) is a circular unitig of one node.
 * SEQUENCE: a unitig of v nodes has k + v - 1 symbols: the first node's k symbols, then the last symbol of every following node.
 * ORDER: ascending by the first node's packed word; the same from run to run and under every knob.
 * TOTALS: with n nodes and U unitigs the symbols total S = n + U (k - 1).
 * The graph is the strand-specific, directed one: a read set from both strands yields each unitig once per strand.  The bidirected
 * (canonical) compaction is out of scope of THIS call: see the canonical unitigs below.
 *
 * Outputs (every buffer may be NULL):
 *   out_offsets     U + 1 words: unitig u is out_symbols[out_offsets[u] .. out_offsets[u + 1]); out_offsets[0] = 0, out_offsets[U] = S
 *   out_symbols     S bytes in the library's symbol codes (A C G T = 1 2 3 5): with the offsets a ragged read set, as it is, for
 *                   msbwt_rle_count_ragged_read_kmers and msbwt_rle_build_from_reads(ascii = 0)
 *   out_count_sums  U words: the sum of count_kmer over the unitig's nodes (mean abundance = the sum / the nodes)
 *   out_ends        U bytes: low nibble = the predecessor bits of the first node, high nibble = the successor bits of the last node: the
 *                   compacted graph's adjacency.  For a circular unitig both nibbles hold exactly the closing edge.
 *   out_flags       U bytes: bit 0 = circular
 * Capacity, as for the dumps: *out_unitigs (NULL: MSBWT_ERR_INVALID_ARG) and *out_symbol_total (may be NULL) are always set; both
 * capacities 0 only counts; otherwise capacity_unitigs < U, or capacity_symbols < S with out_symbols wanted, writes NOTHING, returns
 * MSBWT_ERR_INVALID_ARG and names U and S in the message.  A capacity above need leaves everything past U (U + 1 for the offsets) and
 * past S untouched.  The _device form writes to device buffers on the handle's device -- the byte arrays need no alignment --,
 * synchronises the stream and reports a device fault through msbwt_rle_device_status.
 * A call that fills buffers does the whole work of the counting call again (graph and ranking; no state is kept between calls): a
 * caller who knows bounds -- U <= n, S <= n k -- can make ONE call.
 *
 * How ("Unitigs"): the graph's two walks, the edge pass also keeping each node's predecessor slot; then over the n slots
 * the links, the ranking by pointer jumping over {head, distance} -- double-buffered, stopped when a round leaves nothing unfinished,
 * ceil(log2 n) + 1 rounds at the most --, the opening of isolated cycles by min-label jumping, one scan that numbers the unitigs, and
 * the emission.  Every device loop is bounded by a round count fixed on the host.  Results depend on no knob.
 * Guards, before the first HIP call: NULL handle MSBWT_ERR_INVALID_ARG; nothing loaded MSBWT_ERR_NOT_LOADED ("no BWT loaded"); k
 * outside 1..32 MSBWT_ERR_INVALID_ARG; min_edge below the node threshold and not 0 MSBWT_ERR_INVALID_ARG.  An empty index: U = S = 0.
 * Scratch per call, freed on return (msbwt_rle_device_bytes unchanged); scratch that does not fit: MSBWT_ERR_HIP naming the bytes.
 * msbwt_rle_spectrum_info and msbwt_rle_spectrum_scratch_bytes report the call's writing walk and its scratch as for the graph. */
int msbwt_rle_enumerate_unitigs(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols,
                                uint64_t *out_offsets, uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags,
                                uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t *out_unitigs, uint64_t *out_symbol_total);
int msbwt_rle_enumerate_unitigs_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols,
                                       void *d_out_offsets, void *d_out_count_sums, void *d_out_ends, void *d_out_flags,
                                       uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t *out_unitigs,
                                       uint64_t *out_symbol_total, void *hip_stream);
/* The handle's last unitig call (zeros before the first and after an empty index; a call refused by a guard leaves the words as they
 * were, one refused for its capacities has filled them): [0] nodes, [1] edges, [2] links
 * (closing links of cycles and self-loops included: U + links - circular = nodes), [3] unitigs, [4] symbols, [5] circular unitigs,
 * [6] nodes of the longest unitig, [7] pointer-jumping rounds run (ranking, cycle labels and the ranking of opened cycles together).
 * NULL handle or pointer: MSBWT_ERR_INVALID_ARG. */
#define MSBWT_UNITIG_INFO_WORDS 8
int msbwt_rle_unitig_info(const msbwt_rle *bwt, uint64_t *out /* MSBWT_UNITIG_INFO_WORDS */);
/* Pure function, no device: bytes of HBM a host call over `nodes` nodes that fills all five buffers with `unitigs` unitigs of `symbols`
 * symbols allocates and frees again with the automatic frontier, EXACTLY
 *     msbwt_spectrum_plan(total_rows, free_hbm_bytes, 0, 1)   the walk, the bit per row and the rank checkpoints
 *     + 56 nodes                                              two {head, distance} states of 16 bytes; word, count, predecessor slot
 *     + 16 ceil(nodes / 2048)                                 the numbering scan's two sums per tile of 2048 slots
 *     + 256                                                   the counters, padded
 *     + 8 ceil(nodes / 4)                                     the edge bytes and the link bytes, one each per node, as whole 32-bit words
 *     + 8 unitigs + 256                                       the offsets, U + 1 words, in an allocation of their own, padded
 *     + 8 unitigs                                             the count sums staged for the host
 *     + 8 ceil(symbols / 8)                                   the symbols staged
 *     + 16 ceil(unitigs / 8)                                  the ends and the flags staged
 * Each NULL buffer of the host form takes its staging term less (out_offsets none); the _device form stages nothing: the last three
 * lines less.  A counting call (both capacities 0) allocates the first five lines only, which is what unitigs = symbols = 0 says.
 * MSBWT_ERR_TOO_LARGE from 2^40 rows (or nodes, or unitigs) on; device_bytes may be NULL. */
int msbwt_unitigs_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols,
                       uint64_t *device_bytes);

/* ---- canonical unitigs ---- the strand-merged k-mer graph compacted into its non-branching paths, on the device (no reference
 * counterpart).  Everything follows from count_kmer; rc(x) is the reverse complement of x.
 * CLASSES: for a word x of any length cc(x) = count_kmer(x) + count_kmer(rc(x)), and cc(x) = count_kmer(x) for a palindrome (x = rc(x)):
 * exactly own + other of msbwt_rle_enumerate_canonical_kmers.
 * NODES: all k-mers q with cc(q) >= m = max(min_count, 1) -- both members of every class, a member the index does not hold included.
 * This graph D is closed under rc; with n classes it has N = 2 n - (palindromic nodes) nodes.
 * EDGES: q -> q' (q' = q[1:].c) is an edge when cc(q.c) >= me (min_edge == 0: me = m; 0 < min_edge < m: MSBWT_ERR_INVALID_ARG) AND both
 * q and q' are nodes.  The second clause matters at a palindromic end p, where cc(p) = count_kmer(p) can be below cc(p.c): reads
 * {"CATG"}, k = 2, m = 2 have cc(ATG) = 2 and cc(AT) = 1, so ATG is no edge (even k and m >= 2 only).  D is symmetric: q -> q' exists
 * exactly when rc(q') -> rc(q) does, so in-bit j of q equals out-bit 3 - j of rc(q).
 * LINKS: as above (out(p) = 1 and in(q) = 1), with two cuts: a palindromic node has no links, and an edge whose (k+1)-mer is its own
 * reverse complement (q -> rc(q), odd k) is never a link.  The cuts change links only; edge bits and out_ends keep the real adjacency.
 * With them no path or cycle of D is its own mirror, so the unitigs of D come in pairs {U, rc(U)} of distinct unitigs -- but for a
 * palindromic node, a unitig of one that is its own mirror -- and every class lies in exactly one unitig of a pair exactly once.
 * CHOICE: of a pair, the unitig whose first node's word is smaller is emitted.  A cycle is opened at its smallest word as above; of C and
 * rc(C) the one that holds the smallest word of both is emitted.
 * OUTPUTS: the five arrays of msbwt_rle_enumerate_unitigs with the same meaning, except that out_count_sums holds sums of CLASS counts
 * cc over the unitig's nodes and out_ends is the adjacency in D of the emitted orientation.  ORDER: ascending by first word.
 * TOTALS: S = n + U (k - 1) with n the number of CLASSES.  Results depend on no knob.
 * 1 <= k <= 31, because an edge is a packed (k+1)-mer: k = 32 is MSBWT_ERR_INVALID_ARG.
 *
 * Capacity, NULL buffers, untouched tails, the _device form and its stream, the guards before the first HIP call (with k outside 1..31
 * in place of 1..32), the empty index (U = S = 0) and the scratch (per call, freed on return; one that does not fit: MSBWT_ERR_HIP
 * naming the bytes) are those of msbwt_rle_enumerate_unitigs[_device]; a device fault is reported through msbwt_rle_device_status.
 *
 * How ("Canonical unitigs"): the canonical walk with the window [m, inf) counts and then writes the classes; a kernel
 * writes both member words of every class (a palindrome once) with the class count as the payload, and stable 8-bit radix passes over
 * the low ceil(2k / 8) bytes put the N nodes in word order; word -> slot is a binary search over them.  The four (k+1)-mers out of every
 * node are counted by the packed search, 2^20 nodes a batch, and folded into edge bytes -- cc(q.c) = count(q.c) + count(rc(q.c)), the
 * second read from the mirror node's counts, so every (k+1)-mer word is searched once.  Then the compaction of the unitig call over the
 * N slots, with one kernel behind the links that takes the cut links back and one behind the ranking that marks, of every pair, the
 * unitig that is not emitted; numbering and emission skip those.  Every device loop is bounded by a count fixed on the host. */
int msbwt_rle_enumerate_canonical_unitigs(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols,
                                          uint64_t *out_offsets, uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags,
                                          uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t *out_unitigs,
                                          uint64_t *out_symbol_total);
int msbwt_rle_enumerate_canonical_unitigs_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge,
                                                 void *d_out_symbols, void *d_out_offsets, void *d_out_count_sums, void *d_out_ends,
                                                 void *d_out_flags, uint64_t capacity_unitigs, uint64_t capacity_symbols,
                                                 uint64_t *out_unitigs, uint64_t *out_symbol_total, void *hip_stream);
/* The handle's last canonical unitig call (zeros before the first and after an empty index; a call refused by a guard leaves the words
 * as they were, one refused for its capacities has filled them), for the EMITTED set: [0] classes n, [1] edge classes (the (k+1)-mer
 * classes that are edges of D), [2] links among the emitted unitigs (closing links included: U + links - circular = classes), [3]
 * unitigs U, [4] symbols S, [5] circular unitigs, [6] nodes of the longest unitig, [7] pointer-jumping rounds run; and two words more
 * than msbwt_rle_unitig_info has: [8] palindromic nodes (N = 2 n - [8]), [9] links of D the two cuts took back (both strands counted).
 * NULL handle or pointer: MSBWT_ERR_INVALID_ARG. */
#define MSBWT_CANONICAL_UNITIG_INFO_WORDS 10
int msbwt_rle_canonical_unitig_info(const msbwt_rle *bwt, uint64_t *out /* MSBWT_CANONICAL_UNITIG_INFO_WORDS */);
/* Pure function, no device: bytes of HBM a host call over `classes` classes that fills all five buffers with `unitigs` unitigs of
 * `symbols` symbols allocates and frees again with the automatic frontier, EXACTLY, with slots = 2 classes (the allocation does not
 * wait for the palindromes to be counted):
 *     msbwt_canonical_plan(total_rows, free_hbm_bytes, 0)     the canonical walk: its frontiers and the other strand of a chunk
 *     + 256                                                   the walk's totals, which that plan leaves out
 *     + 128 classes                                           per slot 32 bytes of (k+1)-mer counts -- first the walk's records, later the
 *                                                             two {head, distance} states -- and 32 of (word, class count) twice for the
 *                                                             sort, the free pair of which holds the predecessor slots
 *     + 32 min(slots, 2^20)                                   the (k+1)-mer words of a batch of nodes
 *     + 2048 ceil(slots / 4096)                               the sort's digit histogram per tile of 4096 keys
 *     + 8 (ceil(ceil(slots / 4096) / 4) + 8)                  the levels of its scan
 *     + 16 ceil(slots / 2048)                                 the numbering scan's two sums per tile of 2048 slots
 *     + 512                                                   the counters of the compaction and of this call, padded
 *     + 8 ceil(slots / 4)                                     the edge bytes and the link bytes, one each per slot, as whole 32-bit words
 *     + 8 unitigs + 256 + 8 unitigs + 8 ceil(symbols / 8) + 16 ceil(unitigs / 8)      the second allocation, as in msbwt_unitigs_plan
 * Each NULL buffer of the host form takes its staging term less (out_offsets none); the _device form stages nothing: 8 unitigs + 256
 * is all of the last line.  A counting call (both capacities 0) allocates all but the last line: unitigs = symbols = 0.
 * MSBWT_ERR_TOO_LARGE from 2^40 rows (or classes, or unitigs) on; device_bytes may be NULL. */
int msbwt_canonical_unitigs_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t classes, uint64_t unitigs, uint64_t symbols,
                                 uint64_t *device_bytes);

/* ---- unitig links ---- the edges of the compacted graph: either unitig call with the LINK TABLE behind its five columns, on the device
 * (no reference counterpart).  The five columns are byte for byte those of msbwt_rle_enumerate_unitigs / _canonical_unitigs (but for
 * flag bit 1 below), and msbwt_rle_unitig_info / msbwt_rle_canonical_unitig_info are filled exactly as those calls fill them.
 * SIDES: unitig u has two.  Side 2u leaves u forwards, out of its last node; side 2u + 1 leaves rc(u) forwards, out of the reverse
 * complement of u's first node -- "backwards out of u".
 * ENTRIES: let W be the sequence side a leaves (u or rc(u)).  For every symbol c in A C G T order for which the graph has the edge
 * last(W) -> q' = last(W)[1:].c the side holds one entry 2v + o: v is the returned unitig with q' at an end, o = 0 when q' = first(v),
 * o = 1 when q' = rc(last(v)), o = 0 when both hold.  The entries of a side ascend by c.  q' always lies at an end: an edge that is no
 * link starts at a last node and ends at a first node, the only link that is an entry is the closing link of a circular unitig, and a
 * cut link of the canonical graph is an edge that is no link.
 * PLAIN CALL (the strand-specific graph; rc(u) is no part of it, and a side 2u + 1 is read through the mirrored edges): side 2u has
 * popcount(out_ends[u] >> 4) entries, all even: the successors.  Side 2u + 1 has popcount(out_ends[u] & 15) entries, all odd: 2v + 1
 * for every unitig v whose last node precedes first(u), by DESCENDING predecessor symbol (leaving rc(u) appends the complement).
 * L = 2 (edges - links + circular) of msbwt_rle_unitig_info.  A circular unitig has exactly 2u on side 2u and 2u + 1 on side 2u + 1.
 * CANONICAL CALL (the graph D above): side 2u has popcount(out_ends[u] >> 4) entries, side 2u + 1 popcount(out_ends[u] & 15) -- in-bit
 * j of a node is out-bit 3 - j of its mirror.  A unitig that is its own reverse complement -- a single palindromic node, the only case
 * in which both o apply -- has ONE side: its side 2u + 1 is empty, entries that reach it carry o = 0, and out_flags[u] has bit 1 set
 * (bit 0 stays "circular"; the plain call never sets bit 1).
 * MIRROR RECORDS: write (a, e) for "side a holds entry e", and c(x) = x & ~1 for a unitig that is its own reverse complement, else x.
 * With every (a, e) the table holds (c(e ^ 1), c(a ^ 1)): the same bidirected edge from its other end.  A hairpin edge q -> rc(q) is
 * its own mirror.  Keeping a record only when (a, e) <= its mirror, compared as pairs, keeps every edge once: edges - links + circular
 * records of the plain call (as many as its even sides hold, though not those: the rule keeps (1, 3) and not its mirror (2, 0)),
 * edge_classes - links + circular of the canonical call.
 *
 * Outputs beyond the five columns (every buffer may be NULL):
 *   out_link_offsets  2 U + 1 words: side a is out_link_targets[out_link_offsets[a] .. out_link_offsets[a + 1]); [0] = 0, [2 U] = L
 *   out_link_targets  L words
 * Capacity: the contract of the unitig calls with one capacity more.  *out_unitigs (NULL: MSBWT_ERR_INVALID_ARG), *out_symbol_total and
 * *out_links (each may be NULL) are always set; all three capacities 0 only counts, L included; otherwise capacity_unitigs < U, or
 * capacity_symbols < S with out_symbols wanted, or capacity_links < L with out_link_targets wanted, writes NOTHING, returns
 * MSBWT_ERR_INVALID_ARG and names U, S and L.  Tails past U, U + 1, 2 U + 1, S and L stay untouched.  The _device form writes to device
 * buffers -- the byte arrays need no alignment --, synchronises the stream and reports a device fault through msbwt_rle_device_status.
 * 1 <= k <= 32, canonical 1 <= k <= 31; the guards are those of the unitig calls, in their order, before the first HIP call.  An empty
 * index, or one without a node: U = S = L = 0, and a call with a capacity writes out_link_offsets[0] = 0.  Results depend on no knob.
 *
 * How ("Unitig links"): behind the emission, over the arrays it used.  The tails' degrees are added up for L before a
 * capacity is looked at; then every tail writes its two degrees, one scan (the numbering's helpers, tiles of 2048 words) turns them
 * into offsets, and every tail and head fills its side: a neighbour's word is the node's shifted by a symbol (at k = 32 the successor
 * shifts out of the 64 bits), its slot a binary search over the sorted words of ceil(log2 n) + 1 steps, fixed on the host, and its
 * unitig the number at that slot's head -- or, where the canonical call did not emit that unitig, at the head of its mirror, one more
 * search.  Scratch per call, freed on return; msbwt_rle_spectrum_scratch_bytes reports these calls too. */
int msbwt_rle_enumerate_unitig_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols,
                                     uint64_t *out_offsets, uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags,
                                     uint64_t *out_link_offsets /* 2U + 1 */, uint64_t *out_link_targets /* L */,
                                     uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links,
                                     uint64_t *out_unitigs, uint64_t *out_symbol_total, uint64_t *out_links);
int msbwt_rle_enumerate_unitig_graph_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, void *d_out_symbols,
                                            void *d_out_offsets, void *d_out_count_sums, void *d_out_ends, void *d_out_flags,
                                            void *d_out_link_offsets, void *d_out_link_targets, uint64_t capacity_unitigs,
                                            uint64_t capacity_symbols, uint64_t capacity_links, uint64_t *out_unitigs,
                                            uint64_t *out_symbol_total, uint64_t *out_links, void *hip_stream);
int msbwt_rle_enumerate_canonical_unitig_graph(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge,
                                               uint8_t *out_symbols, uint64_t *out_offsets, uint64_t *out_count_sums, uint8_t *out_ends,
                                               uint8_t *out_flags, uint64_t *out_link_offsets /* 2U + 1 */,
                                               uint64_t *out_link_targets /* L */, uint64_t capacity_unitigs, uint64_t capacity_symbols,
                                               uint64_t capacity_links, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                                               uint64_t *out_links);
int msbwt_rle_enumerate_canonical_unitig_graph_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge,
                                                      void *d_out_symbols, void *d_out_offsets, void *d_out_count_sums, void *d_out_ends,
                                                      void *d_out_flags, void *d_out_link_offsets, void *d_out_link_targets,
                                                      uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links,
                                                      uint64_t *out_unitigs, uint64_t *out_symbol_total, uint64_t *out_links,
                                                      void *hip_stream);
/* Pure functions, no device: bytes of HBM a host call that fills all seven buffers allocates and frees again, EXACTLY
 *     msbwt_unitigs_plan(total_rows, free_hbm_bytes, nodes, unitigs, symbols)   (msbwt_canonical_unitigs_plan for the canonical call)
 *     + 16 unitigs + 256                                      the link offsets, 2 U + 1 words, in a third allocation, padded
 *     + 16 ceil((2 unitigs + 1) / 2048)                       their scan's two sums per tile of 2048 words
 *     + 8 links                                               the link targets staged for the host
 * A NULL out_link_targets, and the _device form, take the last line less.  A counting call (all three capacities 0) allocates what the
 * unitig call's counting call does: unitigs = symbols = links = 0 says so.  MSBWT_ERR_TOO_LARGE as for the unitig plans, and from
 * 2^43 links on; device_bytes may be NULL. */
int msbwt_unitig_graph_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols,
                            uint64_t links, uint64_t *device_bytes);
int msbwt_canonical_unitig_graph_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t classes, uint64_t unitigs, uint64_t symbols,
                                      uint64_t links, uint64_t *device_bytes);

/* ---- unitigs by source ---- the per-input abundance of every unitig: either unitig GRAPH call, on an index with sources attached
 * (msbwt_rle_load_merged_many_sources, msbwt_rle_set_sources), with ONE MORE COLUMN behind the link table (no reference counterpart).
 * The arguments are those of the graph call of the same kind in the same order, out_source_sums behind out_link_targets.
 * S = msbwt_rle_source_count.  Write c_s(q) for the rows of source s in the FM range of the k-mer q, as msbwt_rle_range_sources
 * defines them: the sum of c_s(q) over s is count_kmer(q).
 *   out_source_sums   U x S words, row-major; may be NULL
 * PLAIN CALL: out_source_sums[u S + s] = the sum of c_s(q) over the nodes q of unitig u.
 * CANONICAL CALL: the same sum over the classes of u, a class {q, rc(q)} counting c_s(q) + c_s(rc(q)); a palindromic class
 * (q == rc(q)) counts c_s(q) ONCE.  A member that does not occur in the index adds nothing.
 * ROW SUMS: in both calls row u sums to out_count_sums[u].
 * THRESHOLDS: min_count and min_edge meet the counts over all inputs together, exactly as in the graph calls: the graph is that of
 * the union, and only this column looks at sources.
 * The five columns and the link table are byte for byte what the graph call returns on the same index with the same arguments, and
 * msbwt_rle_unitig_info / msbwt_rle_canonical_unitig_info are filled exactly as those calls fill them.
 * Capacity: the graph call's.  The matrix needs capacity_unitigs >= U and has no capacity of its own; a refused call writes NOTHING,
 * the matrix included, returns MSBWT_ERR_INVALID_ARG and names U, S (symbols) and L; all three capacities 0 only counts; the tail
 * past U x S words stays untouched.  The _device form takes a device pointer.
 * Guards, before the first HIP call: a NULL handle; nothing loaded (MSBWT_ERR_NOT_LOADED, "no BWT loaded"); no attachment
 * (MSBWT_ERR_NOT_LOADED, "no sources attached"); k (1..32, canonical 1..31); the thresholds; *out_unitigs NULL.  An empty index, or
 * one without a node: U = S = L = 0, and a call with a capacity writes out_link_offsets[0] = 0.  Results depend on no knob and are
 * the same from run to run.
 *
 * How ("Unitigs by source"): behind the links, over the arrays the emission used.  The plain call keeps every node's
 * range start from its edge walk; the canonical call searches a chunk of slots' words again for their ranges.  One 8-lane group a
 * slot finds the slot's unitig -- the number at its head, or, where the canonical call did not emit that unitig, at the head of the
 * slot of the word's reverse complement, one binary search --, counts the range's rows per source as the by-source k-mer calls do
 * and adds the non-zero counts to the unitig's row with 64-bit integer atomics. */
int msbwt_rle_enumerate_unitig_graph_by_source(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge, uint8_t *out_symbols,
                                               uint64_t *out_offsets, uint64_t *out_count_sums, uint8_t *out_ends, uint8_t *out_flags,
                                               uint64_t *out_link_offsets /* 2U + 1 */, uint64_t *out_link_targets /* L */,
                                               uint64_t *out_source_sums /* U x S */, uint64_t capacity_unitigs, uint64_t capacity_symbols,
                                               uint64_t capacity_links, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                                               uint64_t *out_links);
int msbwt_rle_enumerate_unitig_graph_by_source_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge,
                                                      void *d_out_symbols, void *d_out_offsets, void *d_out_count_sums, void *d_out_ends,
                                                      void *d_out_flags, void *d_out_link_offsets, void *d_out_link_targets,
                                                      void *d_out_source_sums, uint64_t capacity_unitigs, uint64_t capacity_symbols,
                                                      uint64_t capacity_links, uint64_t *out_unitigs, uint64_t *out_symbol_total,
                                                      uint64_t *out_links, void *hip_stream);
int msbwt_rle_enumerate_canonical_unitig_graph_by_source(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge,
                                                         uint8_t *out_symbols, uint64_t *out_offsets, uint64_t *out_count_sums,
                                                         uint8_t *out_ends, uint8_t *out_flags, uint64_t *out_link_offsets /* 2U + 1 */,
                                                         uint64_t *out_link_targets /* L */, uint64_t *out_source_sums /* U x S */,
                                                         uint64_t capacity_unitigs, uint64_t capacity_symbols, uint64_t capacity_links,
                                                         uint64_t *out_unitigs, uint64_t *out_symbol_total, uint64_t *out_links);
int msbwt_rle_enumerate_canonical_unitig_graph_by_source_device(const msbwt_rle *bwt, size_t k, uint64_t min_count, uint64_t min_edge,
                                                                void *d_out_symbols, void *d_out_offsets, void *d_out_count_sums,
                                                                void *d_out_ends, void *d_out_flags, void *d_out_link_offsets,
                                                                void *d_out_link_targets, void *d_out_source_sums,
                                                                uint64_t capacity_unitigs, uint64_t capacity_symbols,
                                                                uint64_t capacity_links, uint64_t *out_unitigs,
                                                                uint64_t *out_symbol_total, uint64_t *out_links, void *hip_stream);
/* Pure functions, no device: bytes of HBM a host call that fills all eight buffers allocates and frees again, EXACTLY
 *     msbwt_unitig_graph_plan(total_rows, free_hbm_bytes, nodes, unitigs, symbols, links)   (msbwt_canonical_unitig_graph_plan for the
 *                                                                                            canonical call, nodes = classes)
 *     + ceil(8 R / 256) 256                                   the range words: R = nodes, one range start a node (plain call, taken
 *                                                             before its edge walk), or R = 2 min(2 classes, 2^20), a pair {l, h}
 *                                                             a slot of a chunk (canonical call)
 *     + ceil(8 unitigs n_sources / 256) 256                   the matrix staged for the host
 * The _device form takes the last line less; a NULL out_source_sums takes neither line: the call is the graph call then.  A counting
 * call (all three capacities 0) allocates what the graph call's counting call does: unitigs = symbols = links = 0 says so.
 * n_sources outside 1..MSBWT_MERGE_MAX_INPUTS: MSBWT_ERR_INVALID_ARG.  MSBWT_ERR_TOO_LARGE as for the graph plans; device_bytes may
 * be NULL. */
int msbwt_unitig_graph_by_source_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t nodes, uint64_t unitigs, uint64_t symbols,
                                      uint64_t links, size_t n_sources, uint64_t *device_bytes);
int msbwt_canonical_unitig_graph_by_source_plan(uint64_t total_rows, uint64_t free_hbm_bytes, uint64_t classes, uint64_t unitigs,
                                                uint64_t symbols, uint64_t links, size_t n_sources, uint64_t *device_bytes);

/* The bytes of scratch the handle's last k-mer walk call (any call of the four sections above that walks) allocated in HBM and freed
 * again before it returned; 0 before the first one and after a call that allocated nothing (an empty index, a refused argument leaves
 * it as it was).  Every allocation counts with its size, 256 bytes at the least.  For the by-source calls this is what
 * msbwt_kmers_by_source_plan(rows, free, S, records, sorted) says, with records = n for a host dump that asked for counts AND l (8 S or
 * 8 bytes per record less without them) and 0 otherwise, sorted = 1 for a sorted call that fills buffers (a call that only counts marks
 * nothing), plus 8 S n_bins for the spectrum -- the tests hold the two against each other.  NULL handle or pointer: MSBWT_ERR_INVALID_ARG. */
int msbwt_rle_spectrum_scratch_bytes(const msbwt_rle *bwt, uint64_t *out_bytes);

/* ---- traces ---- from each of n seed k-mers, a walk through the k-mer graph, node by node in one direction under one rule, all walks
 * of a batch advancing together on the device (no reference counterpart).  The calls above answer whole-index questions and take
 * scratch in proportion to the nodes; a trace is the LOCAL question -- from this k-mer, where does the graph go? -- and its cost
 * follows the answer, not the index: read correction, bridging between two anchors, local assembly around a k-mer a dump reported.
 * (A "walk" elsewhere in this header is the frontier walk of the enumerating calls; hence "trace".)
 *
 * THE GRAPH is G(k, m, me) exactly as "the k-mer graph" defines it: nodes are the k-mers over ACGT with count_kmer >= m =
 * max(min_count, 1), edges the (k+1)-mers with count_kmer >= me (min_edge == 0: me = m; 0 < min_edge < m: MSBWT_ERR_INVALID_ARG).
 * 1 <= k <= 31: an edge is ONE packed (k+1)-mer, the canonical unitig call's limit and its reason.
 * DIRECTION: MSBWT_TRACE_RIGHT follows successors, MSBWT_TRACE_LEFT predecessors.  The FAN of a node q is the set of edges that leave
 * it in the walk direction (q.c for RIGHT, c.q for LEFT), its BACK-FAN the set of edges that enter it in the walk direction.  With the
 * packed words of "compact queries" (first symbol most significant), for a node word w and a symbol c = 0..3 (A C G T):
 *                 RIGHT                          LEFT
 *   edge word     (w << 2) | c                   (c << 2k) | w
 *   next node     that edge's low 2k bits        (c << 2(k-1)) | (w >> 2)
 * At k = 31 an edge fills all 64 bits.
 * MODE: MSBWT_TRACE_UNIQUE goes on while the fan has exactly one edge.  MSBWT_TRACE_UNITIG does the same and does not enter a node
 * whose back-fan has two or more edges: every step is then a LINK of the unitig section, and a trace from a unitig's first node
 * RIGHT (its last node LEFT) reproduces that unitig of msbwt_rle_enumerate_unitigs.  MSBWT_TRACE_GREEDY takes, at a fan of several
 * edges, the one with the largest count_kmer, on a tie the smallest symbol (A < C < G < T).
 * ONE WALK, with seed s (bits beyond 2k ignored; a target's likewise), cur = s, steps = 0:
 *   0. s is no node: stop NOT_A_NODE with steps = 0.
 *   1. steps == max_steps: stop MAX_STEPS.
 *   2. The fan of cur is empty: stop DEAD_END.
 *   3. The fan has two or more edges and the mode is not GREEDY: stop BRANCH.  Otherwise e is the edge chosen, nxt its other end.
 *   4. Mode UNITIG and the back-fan of nxt has two or more edges: stop MERGE; nxt is not entered.
 *   5. nxt == s: stop RETURNED; nxt is not entered.  An isolated cycle of v nodes ends here after v - 1 steps, a node whose only
 *      edge is its self-loop after 0.
 *   6. Enter nxt: symbols[steps] = the symbol appended (RIGHT) or prepended (LEFT), in the library's codes 1 2 3 5;
 *      edge_sum += count_kmer(e); steps += 1; cur = nxt.
 *   7. Targets were given and cur == target[i]: stop TARGET.  A target is compared with ENTERED nodes only, so a target equal to the
 *      seed never stops a walk.
 *   8. Back to 1.
 * A walk that runs into a cycle that does not hold its seed turns until max_steps: stated, not cured.
 * The full sequence of walk i is the seed followed by its row of symbols (RIGHT), or the row reversed followed by the seed (LEFT).
 *
 * Outputs, every one may be NULL:
 *   out_symbols     n x max_steps bytes, row-major: row i holds out_steps[i] symbols, the rest of the row is left untouched
 *   out_steps       n words
 *   out_stops       n bytes: MSBWT_TRACE_DEAD_END .. MSBWT_TRACE_NOT_A_NODE; 0 is never written
 *   out_edge_sums   n words: the sum of count_kmer over the (k+1)-mers traversed
 *   out_last        n words: the node the walk ended on (the seed, masked, for NOT_A_NODE)
 *   out_fans        n bytes: bit j is set when the edge by symbol j leaves that final node in the walk direction; 0 for NOT_A_NODE.
 *                   What a caller needs to fork at a BRANCH.
 * targets2bit: n words, or NULL.  The _device form takes device pointers, runs on hip_stream, synchronises it before it returns (the
 * scratch is freed then) and reports a device fault through msbwt_rle_device_status, as the enumerating calls do.
 * Guards, before the first HIP call: a NULL handle (MSBWT_ERR_INVALID_ARG); nothing loaded (MSBWT_ERR_NOT_LOADED, "no BWT loaded"); k
 * outside 1..31; a bad min_edge, mode or direction; NULL seeds with n > 0 (all MSBWT_ERR_INVALID_ARG); max_steps, or n x max_steps,
 * from 2^40 on (MSBWT_ERR_TOO_LARGE).  n == 0 and an empty index are MSBWT_OK; on an empty index every stop is NOT_A_NODE.  Results
 * depend on no knob, no index form and no piece, and are the same from run to run.
 *
 * How ("Traces"): the FM index searches in one direction only, so a step cannot reuse the step before it: every edge is
 * a search of its own, and the searches go, a ROUND at a time for all live walks at once, through the packed search of
 * msbwt_rle_count_kmers_packed_device.  Round 0 searches the seeds at length k and their fans; a later round searches, for every live
 * walk, the 4 edges of the fan of the node it is about to enter and, in UNITIG mode, the 4 of its back-fan.  One kernel a round reads
 * the counts, applies steps 4-7 and 1-3, writes a finished walk's outputs once and moves the survivors to the front with their next
 * queries.  The host reads the live count after each round and stops at 0: max_steps + 1 rounds at the most.  The n walks are taken
 * a PIECE at a time (msbwt_rle_set_trace_piece: 0 = automatic, 2^20 walks; results never depend on it), so the scratch does not grow
 * with n.  Queries searched: 5 a walk in round 0, then 4 (UNITIG: 8) a live walk and round; a walk of s steps is live in s later
 * rounds, and in one more where a MERGE or, in UNITIG mode, a RETURNED stops it.  A finished walk is never searched again.
 *
 * msbwt_rle_trace_info: out[MSBWT_TRACE_INFO_WORDS] of the handle's last trace call = [0] walks, [1] rounds run, [2] queries handed to
 * the packed search, [3] steps taken in all, [4] the longest walk, [5] pieces, [6] scratch bytes allocated, [7] walks that were no node.
 * The scratch is per call and freed on return (msbwt_rle_device_bytes unchanged); an empty index and n == 0 allocate nothing.
 * msbwt_trace_plan: pure, no device: [6] of a call on an index that holds something, EXACTLY, with P = min(n, piece), piece 0 = 2^20,
 * and pad(x) = ceil(x / 256) 256:
 *     256                                   the counters
 *     + 2 pad(64 P)                         the walks' states, two buffers
 *     + 2 pad(8 w P)                        the queries and their counts, w = 8 in UNITIG mode, else 5 (round 0 asks 1 + 4 a walk)
 *   and, host != 0 (the _device form's arrays are the caller's own):
 *     + pad(8 P)                            a piece's seeds
 *     + pad(8 P)                            its targets, targets != 0
 *     + pad(P max_steps)                    its rows of symbols
 *     + 3 pad(8 P) + 2 pad(P)               its steps, edge sums and last nodes; its stops and fans
 * A host call stages all six outputs whichever are NULL.  n == 0: 0 bytes.  A bad mode: MSBWT_ERR_INVALID_ARG; MSBWT_ERR_TOO_LARGE as
 * the call; device_bytes may be NULL.
 *
 * Out of scope here: the strand-merged graph, which "canonical traces" below walks; k from 32 on, which needs two words a query; per-source thresholds.
 * All walks between two anchors, forks included, are the "bridges" section's. */
#define MSBWT_TRACE_RIGHT 0
#define MSBWT_TRACE_LEFT 1
#define MSBWT_TRACE_UNIQUE 0
#define MSBWT_TRACE_UNITIG 1
#define MSBWT_TRACE_GREEDY 2
#define MSBWT_TRACE_DEAD_END 1
#define MSBWT_TRACE_BRANCH 2
#define MSBWT_TRACE_MERGE 3
#define MSBWT_TRACE_RETURNED 4
#define MSBWT_TRACE_TARGET 5
#define MSBWT_TRACE_MAX_STEPS 6
#define MSBWT_TRACE_NOT_A_NODE 7
#define MSBWT_TRACE_INFO_WORDS 8
int msbwt_rle_trace_kmers(const msbwt_rle *bwt, const uint64_t *seeds2bit, const uint64_t *targets2bit /* or NULL */, size_t k, size_t n,
                          uint64_t min_count, uint64_t min_edge, int mode, int direction, uint64_t max_steps,
                          uint8_t *out_symbols /* n x max_steps */, uint64_t *out_steps, uint8_t *out_stops, uint64_t *out_edge_sums,
                          uint64_t *out_last, uint8_t *out_fans);
int msbwt_rle_trace_kmers_device(const msbwt_rle *bwt, const void *d_seeds2bit, const void *d_targets2bit /* or NULL */, size_t k, size_t n,
                                 uint64_t min_count, uint64_t min_edge, int mode, int direction, uint64_t max_steps,
                                 void *d_out_symbols, void *d_out_steps, void *d_out_stops, void *d_out_edge_sums, void *d_out_last,
                                 void *d_out_fans, void *hip_stream);
int msbwt_rle_trace_info(const msbwt_rle *bwt, uint64_t *out /* MSBWT_TRACE_INFO_WORDS */);
int msbwt_rle_set_trace_piece(msbwt_rle *bwt, uint64_t walks);
int msbwt_trace_plan(uint64_t n, uint64_t max_steps, int mode, int targets, int host, uint64_t piece, uint64_t *device_bytes);

/* ---- canonical traces ---- the traces above through the strand-merged graph: from each of n seed k-mers a walk through D, on the
 * device (no reference counterpart).  Reads come from both strands, and G sees half the coverage on each: a path seen once per strand
 * is no path of G at min_count = 2, a branch on the other strand goes unseen, and a trace through G does not reproduce the unitigs of
 * msbwt_rle_enumerate_canonical_unitigs.  These calls take the arguments of msbwt_rle_trace_kmers[_device] type for type and return
 * its six outputs; modes, directions and the stops 1-7 are the MSBWT_TRACE_* values, and 1 <= k <= 31.
 *
 * THE GRAPH is D(k, m, me) exactly as "canonical unitigs" defines it.  cc(x) = count_kmer(x) + count_kmer(rc(x)), and cc(x) =
 * count_kmer(x) for a palindrome.  NODES: every k-mer q with cc(q) >= m = max(min_count, 1) -- both members of a class, a member the
 * index does not hold included, so a seed may be a k-mer the index holds only as its reverse complement.  EDGES: q -> q' by symbol c
 * (q.c for RIGHT, c.q for LEFT) when cc of that (k+1)-mer is >= me AND q' is a node; the second clause can fail only at a palindromic
 * q', with k even and m >= 2 (reads {"CATG"}, k = 2, m = 2: cc(CAT) = 2 and cc(AT) = 1, so the fan of CA is empty).  min_edge as above.
 * The FAN, the BACK-FAN, the edge word and the next node are the traces' table, unchanged.
 * ONE WALK: steps 0-8 of "traces" with these changes and no others.
 *   0.  s is no node when cc(s) < m.
 *   2, 3, 4 and out_fans read fans of D: the count is cc, the far end must be a node.
 *   3.  GREEDY takes the edge with the largest cc, on a tie the smallest symbol.
 *   3b. Mode UNITIG only, once e and nxt are chosen: stop MSBWT_CANONICAL_TRACE_MIRROR when cur is a palindrome, nxt is a palindrome, or
 *       e is its own reverse complement; nxt is not entered.  These are exactly the two cuts of the canonical unitigs' LINKS.  The step
 *       comes BEFORE 4: a cut link into a node with two predecessors reports MIRROR, not MERGE.
 *   6.  edge_sum += cc(e).
 *   5, 7 compare words as they are: nxt == s, cur == target.  rc(s) and rc(target) stop nothing.
 * out_last is the word in the walk's orientation; out_edge_sums sums cc.
 * UNIQUE and GREEDY follow D as it is: through palindromic nodes and across hairpin edges q -> rc(q).  After a hairpin the walk runs
 * down the mirror of its own path, until a stop of its own or max_steps: stated, not cured.
 * A UNITIG trace RIGHT from the first node of a unitig of msbwt_rle_enumerate_canonical_unitigs reproduces that unitig, and so does a
 * UNITIG trace LEFT from its last node: steps = nodes - 1, it stops RETURNED exactly on the circular unitigs, and out_fans equals
 * out_ends >> 4 (RIGHT) and out_ends & 15 (LEFT).  For UNIQUE and UNITIG the trace of rc(s) in the other direction is the mirror of the
 * trace of s (symbols complemented, last reverse-complemented, fan bit j <-> 3 - j); GREEDY's tie rule is not symmetric.  An index of
 * the same reads with any of them reverse-complemented returns the same bytes.
 *
 * Guards and their order, the empty index (every stop NOT_A_NODE, seeds masked, nothing allocated), n == 0, NULL outputs, untouched
 * row tails, the _device form and its stream, the scratch (per call, freed on return) and faults through msbwt_rle_device_status are
 * those of msbwt_rle_trace_kmers[_device].  msbwt_rle_set_trace_piece governs both calls.  Results depend on no knob, no index form
 * and no piece.
 *
 * How ("Canonical traces"): the rounds of the traces, with every query searched on both strands.  Round 0 searches the
 * seed and its reverse complement at length k and the 4 edges of the seed's fan with their 4 reverse complements; a later round the
 * same 8 for the candidate's fan and, in UNITIG mode, 8 for its back-fan.  One kernel a round folds the counts to cc (a word that is
 * its own reverse complement counts once), applies the steps, writes a finished walk's outputs once and compacts the survivors with
 * their next queries.  THE NODE CLAUSE: of the four far ends of a fan at most one can be a palindrome -- the one by the complement of
 * the node's second symbol (RIGHT; its last but one for LEFT).  Only with k even and m >= 2 does its count matter; then (E = 1, else
 * E = 0) each walk and fan side asks ONE more query of length k, that far end, searched as a batch of its own; its count is used only
 * where the word is a palindrome.  Queries searched, exactly: (10 + E) n in round 0, then 8 + E (UNITIG: 16 + 2 E) a live walk and
 * round; a walk of s steps is live in s later rounds, and in one more where a MERGE or, in UNITIG mode, a RETURNED stops it.  MIRROR
 * and the RETURNED of the other modes are seen on words and cost no round.
 *
 * msbwt_rle_canonical_trace_info: out[MSBWT_CANONICAL_TRACE_INFO_WORDS] of the handle's last canonical trace call, with the eight
 * meanings of msbwt_rle_trace_info (which a canonical call leaves as it was, and the other way round).
 * msbwt_canonical_trace_plan: pure, no device: msbwt_trace_plan with w = 18 in UNITIG mode, else 11, in its term 2 pad(8 w P) -- [6] of
 * a call on an index that holds something, EXACTLY, whatever k and m are.
 *
 * Out of scope here: k from 32 on; forking at branches; per-source thresholds; a target or the seed matched by its reverse
 * complement; both strands in one extension-count search (that call takes a byte a symbol). */
#define MSBWT_CANONICAL_TRACE_MIRROR 8
#define MSBWT_CANONICAL_TRACE_INFO_WORDS 8
int msbwt_rle_trace_canonical_kmers(const msbwt_rle *bwt, const uint64_t *seeds2bit, const uint64_t *targets2bit /* or NULL */, size_t k,
                                    size_t n, uint64_t min_count, uint64_t min_edge, int mode, int direction, uint64_t max_steps,
                                    uint8_t *out_symbols /* n x max_steps */, uint64_t *out_steps, uint8_t *out_stops,
                                    uint64_t *out_edge_sums, uint64_t *out_last, uint8_t *out_fans);
int msbwt_rle_trace_canonical_kmers_device(const msbwt_rle *bwt, const void *d_seeds2bit, const void *d_targets2bit /* or NULL */, size_t k,
                                           size_t n, uint64_t min_count, uint64_t min_edge, int mode, int direction, uint64_t max_steps,
                                           void *d_out_symbols, void *d_out_steps, void *d_out_stops, void *d_out_edge_sums,
                                           void *d_out_last, void *d_out_fans, void *hip_stream);
int msbwt_rle_canonical_trace_info(const msbwt_rle *bwt, uint64_t *out /* MSBWT_CANONICAL_TRACE_INFO_WORDS */);
int msbwt_canonical_trace_plan(uint64_t n, uint64_t max_steps, int mode, int targets, int host, uint64_t piece, uint64_t *device_bytes);

/* ---- left walks ---- from a BWT row back to the text: batched LF walks, locate and read extraction, on the device (the reference
 * walks one row at a time on the host; msbwt's recoverString and fmlrc's read fetches are this operation).  Every call above goes
 * from a k-mer to the index or from the index to the graph; these go from a row of the index to the reads: which read a row of a
 * k-mer's range [l, h) belongs to and at what offset, and the reads themselves, which an index built by msbwt_rle_build_from_reads or
 * a merge still holds.
 *
 * DEFINITIONS, on the BWT string alone.  S is the decoded BWT of T = msbwt_rle_get_total_size rows, C[c] the rows that hold a symbol
 * below c (the reference's start_index), rank(c, r) the occurrences of c in S[0 .. r), and LF(r) = C[S[r]] + rank(S[r], r), which is
 * below T for every r < T whatever the stream.  ONE WALK from row r_0 with steps = 0:
 *   0. r_0 >= T: stop BAD_ROW with steps = 0; no line of the index is fetched.
 *   1. S[r_steps] == '$' (code 0): stop DOLLAR.  That '$' is neither emitted nor counted.
 *   2. steps == max_steps: stop MAX_STEPS.  (So a walk that stands on a '$' after exactly max_steps steps stops DOLLAR.)
 *   3. symbols[steps] = S[r_steps], a code 1..5 (A C G N T); r_(steps + 1) = LF(r_steps); steps += 1; back to 1.
 * READ AND OFFSET.  Row i < C['A'] = msbwt_rle_get_symbol_count(0), inside the '$' block, is read i: the order of the builder and of
 * naive_bwt -- the reads sorted, duplicates in input order, an empty read first.  A walk from row r that stops DOLLAR after p steps
 * stood at the suffix that starts at offset p of read LF(r_p) = rank('$', r_p); the symbols it emitted are that read's prefix [0, p),
 * LAST SYMBOL FIRST.  The walk from '$'-row i emits read i reversed.  All of it is defined for any loaded stream, whoever built it;
 * on a stream that is no BWT of a read set a walk may never meet a '$' and ends at max_steps.
 *
 * msbwt_rle_walk_rows[_device]: rows = n words.  Outputs, every one may be NULL:
 *   out_symbols   n x max_steps bytes, row-major, in walk order: row i holds out_steps[i] symbols, the rest of the row is left
 *                 untouched.  It needs no alignment.  NULL: the call is LOCATE, and costs the same lines without the stores.
 *   out_steps     n words
 *   out_stops     n bytes: MSBWT_WALK_DOLLAR, MSBWT_WALK_MAX_STEPS or MSBWT_WALK_BAD_ROW; 0 is never written
 *   out_last      n words: r_steps, the row the walk stands on (r_0 for BAD_ROW)
 *   out_reads     n words: the read for a DOLLAR stop, UINT64_MAX otherwise; out_steps is then the offset in it
 * A BAD_ROW also raises MSBWT_ERR_INVALID_RANGE as msbwt_rle_constrain_ranges does -- the host form returns it, the _device form
 * leaves it to msbwt_rle_device_status --; every other walk of the batch is answered all the same.  max_steps == 0 is legal: it tells
 * the rows that hold a '$' from the others.  The _device form takes device pointers, runs on hip_stream, synchronises it before it
 * returns and reports through msbwt_rle_device_status.
 * Guards, in this order, before the first HIP call: a NULL handle (MSBWT_ERR_INVALID_ARG); nothing loaded (MSBWT_ERR_NOT_LOADED, "no
 * BWT loaded"); NULL rows with n > 0 (MSBWT_ERR_INVALID_ARG); max_steps, or n x max_steps, from 2^40 on (MSBWT_ERR_TOO_LARGE).  n == 0
 * and an empty index return MSBWT_OK at once, nothing written.  Results depend on no knob, no index form and no piece.
 *
 * msbwt_rle_extract_reads[_device]: n reads as a ragged set in READING order -- the (symbols, offsets) pair that
 * msbwt_rle_count_ragged_read_kmers and msbwt_rle_build_from_reads (ascii = 0) take as it is.  read_ids: n words, each below
 * msbwt_rle_get_symbol_count(0); NULL: the reads first_read .. first_read + n (first_read is ignored beside read_ids).  An id outside
 * that range is refused with MSBWT_ERR_INVALID_RANGE: by the host form, and for a NULL read_ids by either form, on the host before
 * anything runs; by the _device form through the flags (msbwt_rle_device_status), that read getting length 0.
 * max_len >= 1 bounds every loop on the device: a read longer than max_len yields its LAST max_len symbols and is counted in
 * *out_truncated (may be NULL); a read of exactly max_len symbols is whole.
 *   out_offsets        n + 1 words, written when it is not NULL and the call is not refused for capacity
 *   *out_symbol_total  S, the symbols of the n reads (as extracted); always set, NULL is MSBWT_ERR_INVALID_ARG
 *   out_symbols        NULL: a lengths-only call.  Else capacity_symbols bytes: S of them are written, everything past S is left
 *                      untouched.  capacity_symbols < S: MSBWT_ERR_INVALID_ARG, the message names S, the offsets are left
 *                      untouched, out_symbols is unspecified within its capacity and nothing is written past it.
 * THE WALK IS THE WHOLE COST of a call, and S is not known before it.  A call whose capacity_symbols is at least n x max_len cannot
 * be short and walks ONCE; a call with a smaller capacity walks once for the lengths and, S fitting, once more for the symbols.  So a
 * caller who cannot bound S better than n x max_len allocates that and makes one call; a lengths-only call first buys nothing.
 * Guards, in this order, before the first HIP call: a NULL handle; nothing loaded; max_len == 0 or a NULL out_symbol_total
 * (MSBWT_ERR_INVALID_ARG); max_len, or n x max_len, from 2^40 on (MSBWT_ERR_TOO_LARGE); the ids known on the host
 * (MSBWT_ERR_INVALID_RANGE).  n == 0: S = 0 and out_offsets[0] = 0.
 *
 * How ("Left walks"): one 8-lane group a walk, and ONE 128-byte line a step -- the group reads the symbol at the row out
 * of the line and ranks it from the same registers; an OVERFLOW run block costs one more line.  A walk is a chain of dependent random
 * fetches, so a group keeps four walks in registers side by side, a wave 32 lines in flight.  The step loop runs inside the kernel,
 * max_steps + 1 lines at the most (the last only to see a '$'), and a launch takes a PIECE of the n walks (msbwt_rle_set_walk_piece:
 * 0 = automatic, 2^20 walks, at most 2^28, beyond which MSBWT_ERR_INVALID_ARG; results never depend on it), so that the scratch does
 * not grow with n.  Extraction walks a piece into rows of max_len bytes, scans the lengths with the running base carried from piece to
 * piece, and one kernel turns every row round into its ragged place.  A walk costs the offset inside the read, which is right for short reads; there is no sampled
 * suffix array, and on long-read indexes max_steps bounds what a locate may cost.
 *
 * msbwt_rle_walk_info: out[MSBWT_WALK_INFO_WORDS] of the handle's last call of either kind = [0] walks, [1] steps taken in all,
 * [2] DOLLAR stops, [3] MAX_STEPS stops (extraction: the truncated reads), [4] BAD_ROW stops, [5] pieces launched, [6] scratch bytes
 * allocated, [7] microseconds; an extraction that walked twice reports its second walk in [1]-[4] and the pieces of both in [5].  The scratch is per call and freed on return
 * (msbwt_rle_device_bytes unchanged); n == 0 and an empty index allocate nothing.
 * msbwt_walk_plan: pure, no device: [6] of a msbwt_rle_walk_rows[_device] call on an index that holds something, EXACTLY, with
 * P = min(n, piece), piece 0 = 2^20, and pad(x) = ceil(x / 256) 256:
 *     256                                   the counters -- all the _device form allocates
 *   and, host != 0:
 *     + 4 pad(8 P) + pad(P)                 a piece's rows, steps, last rows and reads; its stops -- staged whichever are NULL
 *     + pad(P max_steps)                    its rows of symbols, symbols != 0 (out_symbols is not NULL)
 * n == 0: 0 bytes.  A piece above 2^28: MSBWT_ERR_INVALID_ARG; MSBWT_ERR_TOO_LARGE as the call; device_bytes may be NULL.
 * [6] of a msbwt_rle_extract_reads[_device] call with n > 0, EXACTLY, whether it walks once or twice (P as above, max_len for
 * max_steps):
 *     256                                   the counters
 *     + pad(8 (P + 1))                      the lengths of a piece, and one word behind them
 *     + pad(8 w)                            their scan's sums: w = 1, and with x = P + 1, while x > 2048: x = ceil(x / 2048), w += x
 *     + pad(P max_len)                      the walk-order rows, out_symbols not NULL
 *   and in the host form:
 *     + pad(8 P)                            a piece's ids, read_ids not NULL
 *     + pad(8 (P + 1))                      its offsets, out_offsets not NULL
 *     + pad(P max_len)                      its symbols, out_symbols not NULL
 *
 * Out of scope here: a sampled suffix array; right walks; per-source filtering of the located reads (index the source vector with
 * out_reads); forms for several GPUs. */
/* (Indented inside a guard, not at the line's start as elsewhere in this header: tests/test_canonical_trace_abi.py takes every line
 * from "canonical traces" to "several GPUs" that starts with "#define" for a constant of that section.) */
#ifndef MSBWT_WALK_INFO_WORDS
#  define MSBWT_WALK_DOLLAR 1
#  define MSBWT_WALK_MAX_STEPS 2
#  define MSBWT_WALK_BAD_ROW 3
#  define MSBWT_WALK_INFO_WORDS 8
#endif
int msbwt_rle_walk_rows(const msbwt_rle *bwt, const uint64_t *rows, size_t n, uint64_t max_steps, uint8_t *out_symbols /* n x max_steps */,
                        uint64_t *out_steps, uint8_t *out_stops, uint64_t *out_last, uint64_t *out_reads);
int msbwt_rle_walk_rows_device(const msbwt_rle *bwt, const void *d_rows, size_t n, uint64_t max_steps, void *d_out_symbols, void *d_out_steps,
                               void *d_out_stops, void *d_out_last, void *d_out_reads, void *hip_stream);
int msbwt_rle_extract_reads(const msbwt_rle *bwt, const uint64_t *read_ids /* or NULL */, uint64_t first_read, size_t n, uint64_t max_len,
                            uint8_t *out_symbols, uint64_t *out_offsets /* n + 1 */, uint64_t capacity_symbols, uint64_t *out_symbol_total,
                            uint64_t *out_truncated);
int msbwt_rle_extract_reads_device(const msbwt_rle *bwt, const void *d_read_ids /* or NULL */, uint64_t first_read, size_t n, uint64_t max_len,
                                   void *d_out_symbols, void *d_out_offsets, uint64_t capacity_symbols, uint64_t *out_symbol_total,
                                   uint64_t *out_truncated, void *hip_stream);
int msbwt_rle_walk_info(const msbwt_rle *bwt, uint64_t *out /* MSBWT_WALK_INFO_WORDS */);
int msbwt_rle_set_walk_piece(msbwt_rle *bwt, uint64_t walks);
int msbwt_walk_plan(uint64_t n, uint64_t max_steps, int symbols, int host, uint64_t piece, uint64_t *device_bytes);

/* ---- read overlaps ---- the suffix-prefix overlaps of queries with the reads of the index, every length from ONE backward search,
 * batched on the device (the reference has no counterpart: it answers one constrain_range at a time on the host).  Suffix-prefix
 * overlaps between reads are the edges of a string graph (Simpson and Durbin's FM-index overlapper), the seeds of read-to-read
 * correction, and the test for "does this contig end continue into a read".  msbwt_rle_extract_reads -> msbwt_rle_read_overlaps is an
 * all-against-all overlap of an index whose reads are gone.
 *
 * DEFINITIONS, on the BWT string alone; they hold on any loaded stream, whoever built it.  S, T, C[c] and rank(c, r) are as in the
 * "left walks" section, and constrain(c, [l, h)) = [C[c] + rank(c, l), C[c] + rank(c, h)).  A query is a string Q of L >= 0 symbol
 * codes.  The call takes min_overlap = m >= 1, max_overlap = M (0 means no limit) and strand (0: Q as given; 1: its reverse
 * complement, COMPLEMENT_INT = [0,5,3,2,4,1], N stays N).  Let Q' be the string actually searched and E = min(L, M) (E = L when M is
 * 0).  Set R_0 = [0, T) and j = 0.
 *   1. If j >= m and D_j = [rank('$', l_j), rank('$', h_j)) is not empty, emit the record (j, D_j.l, D_j.h - D_j.l).
 *   2. If j == E, stop END.
 *   3. Let c = Q'[L - 1 - j].  If c is 0 or above 5, stop BAD_SYMBOL.  The records emitted so far stand.
 *   4. Set R_(j+1) = constrain(c, R_j).  If it is empty, stop EMPTY.  Otherwise set j += 1 and go back to 1.
 * After j symbols [l_j, h_j) holds the suffixes that start with the last j symbols of Q'; the rows among them whose BWT symbol is '$'
 * are the reads that BEGIN with those j symbols, and row i of the '$' block is read i of the sorted read set: D_j is a contiguous
 * interval of read ids, every read whose prefix equals that suffix of Q'.  Per query the call returns its records, in ascending j;
 * `matched`, the final j: the longest suffix of Q', up to E symbols, that occurs in the index; `edges`, the sum of the counts of its
 * records; and the stop code.  A record of length j == L names the reads that start with all of Q: Q itself and its duplicates when
 * they are in the index, and every read that contains Q as a prefix.  The call reports them; dropping self, duplicate and containment
 * edges is the caller's policy.  An index of T = 0 rows answers before any search: every query stops EMPTY with matched = 0 and no
 * records, and nothing is allocated.
 *
 * msbwt_rle_read_overlaps[_device]: the n queries are symbol codes as a ragged set, the (reads, read_offsets) pair of
 * msbwt_rle_extract_reads; they need no alignment.  Outputs, every one may be NULL unless stated:
 *   out_offsets          n + 1 words: the records of query i are [out_offsets[i], out_offsets[i + 1]) of the three columns
 *   out_lengths, out_first, out_counts   the record columns, capacity_records words each: all three, or none
 *   *out_record_total    R, the records of all queries; always set, NULL is MSBWT_ERR_INVALID_ARG
 *   out_matched, out_edges   n words each;  out_stops  n bytes: MSBWT_OVERLAP_END, _EMPTY or _BAD_SYMBOL; 0 is never written
 * All three columns NULL is a COUNTING call: one search, and every per-query output is written.  A FILLING call costs TWO searches:
 * pass A writes the per-query outputs and counts the records, a scan places them, pass B searches again and writes each record at
 * its place; everything past R is left untouched.  (A single pass through a fixed-stride staging area is a follow-up.)
 * capacity_records < R: MSBWT_ERR_INVALID_ARG, the message names R; the per-query outputs are written all the same, the columns are
 * unspecified within their capacity and nothing is written past it.  A BAD_SYMBOL also raises MSBWT_ERR_INVALID_SYMBOL as a BAD_ROW
 * raises its error in msbwt_rle_walk_rows -- the host form returns it, the _device form leaves it to msbwt_rle_device_status --;
 * every other query is answered all the same.  The _device form takes device pointers (out_record_total a host pointer), runs on
 * hip_stream, synchronises it before it returns and reports through msbwt_rle_device_status; read_offsets that decrease show there as
 * MSBWT_ERR_INVALID_RANGE, that query searched as an empty one.
 * Guards, in this order, before the first HIP call: a NULL handle (MSBWT_ERR_INVALID_ARG); nothing loaded (MSBWT_ERR_NOT_LOADED, "no
 * BWT loaded"); NULL reads or read_offsets with n > 0, a NULL out_record_total, min_overlap == 0, a strand that is not 0 or 1, or only
 * some of the three columns given (MSBWT_ERR_INVALID_ARG); n from 2^40 on (MSBWT_ERR_TOO_LARGE: before an offset is read); host form
 * only: offsets that decrease (MSBWT_ERR_INVALID_RANGE), then symbols from 2^40 on (MSBWT_ERR_TOO_LARGE).  n == 0 returns MSBWT_OK
 * with R = 0 and out_offsets[0] = 0.  Results depend on no knob, no index form and no piece.
 *
 * How ("Read overlaps"): one 8-lane group a query, four queries a group side by side, because a search is a chain of
 * dependent random fetches.  A step fetches the line of l_j and the line of h_j -- ONE line when both bounds lie in the same block,
 * none for a bound that is T -- and takes from those registers the ranks of the next symbol AND of '$': both ranks sit in the same
 * 128-byte lines the search step fetches anyway.  Step 0 needs no line.  A search fetches at most 2 matched + 2 lines, plus at most
 * one more per bound that lies in an OVERFLOW run block.  The step loop runs inside the kernel, and a launch takes a PIECE of the n
 * queries (msbwt_rle_set_overlap_piece: 0 = automatic, 2^20 queries, at most 2^28, beyond which MSBWT_ERR_INVALID_ARG).  Pair blocks
 * and the direct and sparse tables are left out of this version.
 *
 * msbwt_rle_overlap_info: out[MSBWT_OVERLAP_INFO_WORDS] of the handle's last call = [0] queries, [1] symbols consumed in all (the sum
 * of matched), [2] records, [3] edges, [4] END stops, [5] EMPTY stops, [6] BAD_SYMBOL stops, [7] index lines fetched (both passes),
 * [8] pieces, [9] scratch bytes at their peak, [10] microseconds, [11] the most symbols a piece staged, [12] the most records a piece
 * staged ([11], [12]: host form, else 0).  The scratch is per call and freed on return (msbwt_rle_device_bytes unchanged).
 * msbwt_overlap_plan: pure, no device: [9] of a call with n > 0 on an index that holds something, EXACTLY, with P = min(n, piece),
 * piece 0 = 2^20, pad(x) = ceil(x / 256) 256, piece_symbols = [11] and piece_records = [12] of that call (the most symbols the queries
 * of one piece hold; the most records one piece emits, 0 for a counting call):
 *     256                                   the counters
 *     + pad(8 (P + 1))                      the record counts of a piece, and one word behind them
 *     + pad(8 w)                            their scan's sums: w = 1, and with x = P + 1, while x > 2048: x = ceil(x / 2048), w += x
 *   and, host != 0 (piece_symbols and piece_records are ignored otherwise):
 *     + 2 pad(8 (P + 1))                    a piece's query offsets and record offsets
 *     + 2 pad(8 P) + pad(P)                 its matched and edges; its stops -- staged whichever are NULL
 *     + pad(piece_symbols)                  its symbols
 *     + 3 pad(8 piece_records)              its record columns, piece_records > 0
 * n == 0: 0 bytes.  A piece above 2^28: MSBWT_ERR_INVALID_ARG; n, piece_symbols or piece_records from 2^40 on: MSBWT_ERR_TOO_LARGE;
 * device_bytes may be NULL.
 *
 * Out of scope here: the pair blocks and tables under the first symbols of a search; a single-pass filling call; forms for several
 * GPUs. */
#ifndef MSBWT_OVERLAP_INFO_WORDS
#  define MSBWT_OVERLAP_END 1
#  define MSBWT_OVERLAP_EMPTY 2
#  define MSBWT_OVERLAP_BAD_SYMBOL 3
#  define MSBWT_OVERLAP_INFO_WORDS 13
#endif
int msbwt_rle_read_overlaps(const msbwt_rle *bwt, const uint8_t *reads, const uint64_t *read_offsets /* n + 1 */, size_t n, uint64_t min_overlap,
                            uint64_t max_overlap, int strand, uint64_t *out_offsets /* n + 1 */, uint64_t *out_lengths, uint64_t *out_first,
                            uint64_t *out_counts, uint64_t capacity_records, uint64_t *out_record_total, uint64_t *out_matched, uint64_t *out_edges,
                            uint8_t *out_stops);
int msbwt_rle_read_overlaps_device(const msbwt_rle *bwt, const void *d_reads, const void *d_read_offsets, size_t n, uint64_t min_overlap,
                                   uint64_t max_overlap, int strand, void *d_out_offsets, void *d_out_lengths, void *d_out_first, void *d_out_counts,
                                   uint64_t capacity_records, uint64_t *out_record_total, void *d_out_matched, void *d_out_edges, void *d_out_stops,
                                   void *hip_stream);
int msbwt_rle_overlap_info(const msbwt_rle *bwt, uint64_t *out /* MSBWT_OVERLAP_INFO_WORDS */);
int msbwt_rle_set_overlap_piece(msbwt_rle *bwt, uint64_t queries);
int msbwt_overlap_plan(uint64_t n, int host, uint64_t piece, uint64_t piece_symbols, uint64_t piece_records, uint64_t *device_bytes);

/* ---- bridges ---- all bounded walks of the k-mer graph between two anchor k-mers, for n pairs (seed, target) at once, on the device
 * (no reference counterpart).  This is what an fmlrc-style corrector does for every weak stretch of a read: two solid k-mers flank the
 * stretch, and every walk of the graph that leads from one into the other within a window of lengths and a branching budget is a
 * candidate for what the read should say there.  A trace follows one rule along one path and stops at the first BRANCH; a bridge call
 * explores the branches, level by level.
 *
 * THE GRAPH G(k, m, me), the thresholds (min_count, min_edge), the packed words, the edge word, the next node and the two directions
 * are exactly those of "traces", 1 <= k <= 31; MSBWT_BRIDGE_RIGHT and MSBWT_BRIDGE_LEFT have the numbers of the traces' directions.
 * As there me >= m, so the far end of an edge is always a node.  A WALK may repeat nodes, the seed included.
 * ONE PAIR i, with seed s and target t (bits beyond 2k ignored in both), lo = max(min_steps, 1), found = 0:
 *   0. s is no node: stop NO_SEED.  Else t is no node: stop NO_TARGET.  In both cases found = 0 and depth = 0.
 *   1. W(0) = {the empty walk standing on s}.  For r = 1, 2, ...:
 *      EXPAND.   max_steps == 0: stop MAX_STEPS with depth 0.  Otherwise E(r) is every extension of every walk of W(r-1) by one edge
 *                of its last node's fan.  E(r) keeps the order of W(r-1) and, within one parent, the order A < C < G < T: every level
 *                is in lexicographic order of its rows of symbols.
 *      COLLECT.  B(r) is the members of E(r) whose new node equals t, when r >= lo: the bridges of length r.  They are numbered found,
 *                found + 1, ... in that order, and those numbered below max_paths are written.  Then found += |B(r)|,
 *                W(r) = E(r) \ B(r), and depth = r.  An entry into t with r < lo does not end the walk.
 *      STOP, in this precedence: found >= max_paths: FULL.  W(r) is empty: EXHAUSTED.  r == max_steps: MAX_STEPS.
 *                |W(r)| > max_live: TOO_WIDE.  Otherwise go on.
 * Whatever the stop, THE BRIDGES OF LENGTH <= out_depths[i] ARE ALL COUNTED IN out_found[i], and the first min(found, max_paths) of
 * them, in the order (length, then symbols), are the ones written.  EXHAUSTED says in addition that no longer bridge exists.  A walk
 * that enters t at r >= lo ends there: a bridge is never extended through its target.
 * The full sequence of bridge (i, j) is the seed followed by its row of symbols (RIGHT), or the row reversed followed by the seed (LEFT).
 *
 * Outputs, every one may be NULL; with out_symbols NULL the call is a COUNTING call:
 *   out_symbols     n x max_paths x max_steps bytes: row (i, j) holds out_lengths[i max_paths + j] symbols in walk order, in the
 *                   library's codes 1 2 3 5; the rest of the row, and every unused row, is left untouched
 *   out_lengths     n x max_paths words: the length of bridge (i, j); unused entries are written 0
 *   out_edge_sums   n x max_paths words: the sum of count_kmer over the (k+1)-mers of bridge (i, j); unused entries are written 0
 *   out_found       n words;  out_depths  n words: the last level collected;  out_live  n words: |W(depth)| at the stop (0 for NO_SEED
 *                   and NO_TARGET, 1 for max_steps == 0)
 *   out_stops       n bytes: MSBWT_BRIDGE_EXHAUSTED .. MSBWT_BRIDGE_NO_TARGET; 0 is never written
 * The _device form takes device pointers, runs on hip_stream, synchronises it before it returns (the scratch is freed then) and
 * reports a device fault through msbwt_rle_device_status, as the trace calls do.
 * Guards, before the first HIP call: those of the traces (a NULL handle; nothing loaded, MSBWT_ERR_NOT_LOADED; k outside 1..31; a bad
 * min_edge or direction; NULL seeds with n > 0); NULL targets with n > 0, max_paths == 0, max_live == 0, min_steps > max_steps (all
 * MSBWT_ERR_INVALID_ARG); max_steps above MSBWT_BRIDGE_MAX_STEPS_CAP, max_live above MSBWT_BRIDGE_MAX_LIVE_CAP, n x max_paths or
 * n x max_paths x max_steps from 2^40 on (MSBWT_ERR_TOO_LARGE).  n == 0 and an empty index are MSBWT_OK; on an empty index every
 * stop is NO_SEED.  Results depend on no knob, no index form and no piece size, and are the same from run to run -- which bridges are
 * written, and in which row, included.
 *
 * How ("Bridges"): rounds of the packed search of msbwt_rle_count_kmers_packed_device, as the traces'.  Round 0 searches
 * every pair's seed and target at length k and the seed's fan at k + 1.  The FRONTIER is one array of fixed-size states in the order
 * (pair, walk order): pair, node, steps, edge sum and the walk's symbols at 2 bits, 64 + 8 ceil(max_steps / 32) bytes.  A round
 * searches the 4 edges of every state's fan, then: a kernel forms every state's child and bridge masks and adds them up per pair (64-bit
 * atomic adds: order-free sums), a kernel applies the four stops per pair, a STABLE exclusive scan over the states' child and bridge
 * counts gives every child its slot and every bridge its number, and a kernel writes the children -- with their 4 next queries -- to the
 * other buffer and the bridges to their rows.  No atomic ticket decides an order, so run-to-run sameness needs no sort.  The host
 * reads the size of the next level once a round.  The n pairs are taken a PIECE at a time: P = max(1, slots / max_live) pairs, slots
 * from msbwt_rle_set_bridge_slots (0 = automatic: 2^20; max_live where that is larger; at most 2^28, beyond which
 * MSBWT_ERR_INVALID_ARG) -- a pair that goes on holds at most max_live states, so a piece's frontier never outgrows its P max_live slots.
 * Queries searched, EXACTLY: 6 a pair in round 0, then 4 a state of every W(r) that goes on.
 *
 * msbwt_rle_bridge_info: out[MSBWT_BRIDGE_INFO_WORDS] of the handle's last bridge call = [0] pairs, [1] rounds run (round 0 and every
 * expansion, summed over the pieces), [2] queries handed to the packed search, [3] walk-steps expanded (the sum of |E(r)|), [4] bridges
 * found, [5] pieces, [6] scratch bytes allocated, [7] the widest frontier of a piece (its pairs in round 0, else the states of a
 * level).  The scratch is per call and freed on return (msbwt_rle_device_bytes unchanged); an empty index and n == 0 allocate nothing.
 * msbwt_bridge_plan: pure, no device: [6] of a call on an index that holds something, EXACTLY, with s = max(slots, max_live) (slots 0 =
 * 2^20), P = min(n, s / max_live), S = P max_live, W = 8 + ceil(max_steps / 32) and pad(x) = ceil(x / 256) 256:
 *     256                                   the counters
 *     + pad(48 P)                           the pairs' table
 *     + 2 pad(8 W S)                        the states, two buffers
 *     + pad(8 S)                            a scan word a state
 *     + pad(8 w)                            the scan's sums: w = 1, and with x = S, while x > 2048: x = ceil(x / 2048), w += x
 *     + 2 pad(8 max(4 S, 6 P))              the queries and their counts
 *   and, host != 0 (the _device form's arrays are the caller's own):
 *     + 2 pad(8 P)                          a piece's seeds and targets
 *     + pad(P max_paths max_steps)          its rows of symbols
 *     + 2 pad(8 P max_paths)                its lengths and edge sums
 *     + 3 pad(8 P) + pad(P)                 its found, depths and live; its stops
 * A host call has room for all seven outputs whichever are NULL.  n == 0: 0 bytes.  max_paths == 0, max_live == 0 or slots above 2^28:
 * MSBWT_ERR_INVALID_ARG; MSBWT_ERR_TOO_LARGE as the call; device_bytes may be NULL.
 *
 * Out of scope here: the strand-merged graph; k from 32 on; choosing among bridges by edit distance to the read; per-source
 * thresholds; forms for several GPUs. */
#ifndef MSBWT_BRIDGE_INFO_WORDS
#  define MSBWT_BRIDGE_RIGHT 0
#  define MSBWT_BRIDGE_LEFT 1
#  define MSBWT_BRIDGE_EXHAUSTED 1
#  define MSBWT_BRIDGE_FULL 2
#  define MSBWT_BRIDGE_MAX_STEPS 3
#  define MSBWT_BRIDGE_TOO_WIDE 4
#  define MSBWT_BRIDGE_NO_SEED 5
#  define MSBWT_BRIDGE_NO_TARGET 6
#  define MSBWT_BRIDGE_MAX_STEPS_CAP 4096
#  define MSBWT_BRIDGE_MAX_LIVE_CAP 16777216
#  define MSBWT_BRIDGE_INFO_WORDS 8
#endif
int msbwt_rle_bridge_kmers(const msbwt_rle *bwt, const uint64_t *seeds2bit, const uint64_t *targets2bit, size_t k, size_t n, uint64_t min_count,
                           uint64_t min_edge, int direction, uint64_t min_steps, uint64_t max_steps, uint64_t max_paths, uint64_t max_live,
                           uint8_t *out_symbols /* n x max_paths x max_steps */, uint64_t *out_lengths /* n x max_paths */,
                           uint64_t *out_edge_sums /* n x max_paths */, uint64_t *out_found, uint8_t *out_stops, uint64_t *out_depths,
                           uint64_t *out_live);
int msbwt_rle_bridge_kmers_device(const msbwt_rle *bwt, const void *d_seeds2bit, const void *d_targets2bit, size_t k, size_t n, uint64_t min_count,
                                  uint64_t min_edge, int direction, uint64_t min_steps, uint64_t max_steps, uint64_t max_paths, uint64_t max_live,
                                  void *d_out_symbols, void *d_out_lengths, void *d_out_edge_sums, void *d_out_found, void *d_out_stops,
                                  void *d_out_depths, void *d_out_live, void *hip_stream);
int msbwt_rle_bridge_info(const msbwt_rle *bwt, uint64_t *out /* MSBWT_BRIDGE_INFO_WORDS */);
int msbwt_rle_set_bridge_slots(msbwt_rle *bwt, uint64_t slots);
int msbwt_bridge_plan(uint64_t n, uint64_t max_steps, uint64_t max_paths, uint64_t max_live, int host, uint64_t slots, uint64_t *device_bytes);

/* ---- several GPUs of one node (no reference counterpart: the crate is single-threaded) ----
 * count_kmer calls are independent and read-only (`&self`, src/msbwt_core.rs:125), so the path
 * shards over queries: every device holds a replica of the index, a batch is cut into contiguous
 * shards that start at multiples of 16 queries, and the counts of all shards end up in ONE buffer.
 *
 * msbwt_rle_replicate: a new, independent handle on `device` holding a copy of src's loaded index --
 * blocks, suffix table, presence filter and pair index travel GPU -> GPU (hipMemcpyPeerAsync: over
 * xGMI when peer access is available) instead of being uploaded and rebuilt per device.  NULL on
 * error (msbwt_rle_last_error(src) says why).  `device` may equal src's own (tests). */
msbwt_rle *msbwt_rle_replicate(const msbwt_rle *src, int device);
/* Host batch over `n_replicas` handles (normally one per GPU; replicas[0] may be the original):
 * one host thread and one pinned pipeline per replica, each shard's counts are copied straight
 * into out_counts -- no collective is needed.  Same arguments and results as
 * msbwt_rle_count_kmers / msbwt_rle_count_read_kmers on a single handle. */
int msbwt_rle_count_kmers_multi(const msbwt_rle *const *replicas, size_t n_replicas, const uint8_t *kmers,
                                size_t k, size_t n, uint64_t *out_counts);
int msbwt_rle_count_read_kmers_multi(const msbwt_rle *const *replicas, size_t n_replicas, const uint8_t *reads,
                                     size_t read_len, size_t n_reads, size_t k, int ascii, uint64_t *out_fwd,
                                     uint64_t *out_rc);
/* Device batch: d_kmers and d_out_counts live on replicas[0]'s device.  Shard r is copied to
 * replica r's device, counted there and its counts are copied back into d_out_counts, all by peer
 * copies on that replica's stream (the gather over xGMI).  Synchronous: d_kmers must be complete
 * before the call, d_out_counts is complete when it returns. */
int msbwt_rle_count_kmers_multi_device(const msbwt_rle *const *replicas, size_t n_replicas, const void *d_kmers,
                                       size_t k, size_t n, void *d_out_counts);

/* ---- one process per GPU (the shape `bench.py --gpus N` and an MPI-style Rust host use): every rank holds its
 * own handle with a full index, counts its shard of the batch with msbwt_rle_count_kmers_device, and ONE
 * collective leaves every rank with all counts -- ncclAllGather over RCCL / xGMI, the only exchange step of this
 * path (queries are `&self`, src/msbwt_core.rs:125: no rank needs anything from another one before that).
 * librccl.so is bound at run time (an RCCL already mapped into the process, e.g. PyTorch's, is shared);
 * without it these calls return MSBWT_ERR_RCCL.
 *
 * Communicator bootstrap, for hosts that do not link RCCL themselves: rank 0 obtains an id
 * (MSBWT_COMM_ID_BYTES opaque bytes), hands it to the other ranks by whatever channel the host has (a file, MPI,
 * an environment variable), and every rank calls msbwt_comm_init_rank with its GPU current.  A communicator the
 * host created itself (ncclComm_t) is accepted just as well. */
#define MSBWT_COMM_ID_BYTES 128
int msbwt_comm_get_unique_id(void *out_id);
int msbwt_comm_init_rank(void **out_comm, int nranks, const void *id, int rank);
int msbwt_comm_destroy(void *comm);
/* d_all[r * n_mine + i] = rank r's d_mine[i] (u64 counts, device pointers on the handle's device; every rank
 * passes the same n_mine -- pad the last shard), asynchronous on `hip_stream`.  wire_bits = 64, or 32 / 16: the
 * counts travel narrowed and are widened on arrival (8 bytes per count over xGMI can cost more than the search
 * itself); a count that does not fit makes msbwt_rle_device_status return MSBWT_ERR_OVERFLOW -- repeat the
 * gather with 64.  Calls on one handle must be ordered by the caller (one stream): they share scratch memory. */
int msbwt_rle_allgather_counts(const msbwt_rle *bwt, void *comm, const void *d_mine, size_t n_mine, void *d_all, int wire_bits,
                               void *hip_stream);

/* ONE batch counted and gathered as a pipeline.  A caller that counts its shard with msbwt_rle_count_kmers_device and then calls
 * msbwt_rle_allgather_counts sees kernel + gather + widening one after the other (a steady stream of batches hides the gather behind the
 * next batch's kernel; a single batch cannot).  This call cuts the rank's shard of n_mine queries into `pieces` (1..64; pieces of whole
 * 16-query units) and searches piece i on hip_stream while the counts of piece i - 1 travel -- narrowed to wire_bits, ncclAllGather,
 * put at their place -- on a second stream of the handle; hip_stream continues when the last piece has arrived.
 * d_kmers: n_mine x k symbol codes (this rank's shard); d_mine_counts: n_mine u64 (this rank's counts, also an output);
 * d_all[r * n_mine + i] = rank r's count i as out_bits-wide unsigned integers: 64, or the wire width ("narrow at destination": no
 * widening pass and an array a quarter or half the size -- 8 GB less to write for the 10^9-query line of BASELINE configs[4]).
 * Every rank passes the same n_mine, wire_bits, out_bits and pieces.  A count that does not fit the wire width makes
 * msbwt_rle_device_status return MSBWT_ERR_OVERFLOW.  Calls on one handle must be ordered by the caller (they share scratch). */
int msbwt_rle_count_kmers_allgather_device(const msbwt_rle *bwt, void *comm, const void *d_kmers, size_t k, size_t n_mine, void *d_mine_counts,
                                           void *d_all, int wire_bits, int out_bits, int pieces, void *hip_stream);
/* How that call cuts a shard (a pure function, no device needed): queries per piece -- whole 16-query units, at most `pieces` pieces
 * for any n_mine, the last one takes what is left. */
size_t msbwt_allgather_piece_queries(size_t n_mine, int pieces);

/* ---- batch order (no reference counterpart) ----
 * The order in which a batch is handed over does not change a single count, but it changes how fast they come: a batch whose
 * k-mers are ordered by (their last 17 symbols as a string, then the symbols before those going leftwards) keeps neighbouring
 * queries on neighbouring index lines through the search -- measured up to 2.0x on dense batches over the DIRECT suffix table
 * (10^8 read-derived 31-mers over a 2 x 10^9-symbol BWT, rounds 3-4).  msbwt_kmer_order_keys hands out the 64-bit key to sort by
 * (ascending), for callers that hold a sorted k-mer list anyway or count a batch more than once.
 * kmers: n x k symbol codes; a '$' / 'N' / invalid symbol among the (at most 31) symbols the key reads gives UINT64_MAX. */
int msbwt_kmer_order_keys(const uint8_t *kmers, size_t k, size_t n, uint64_t *out_keys);
/* The library can also order a batch itself, inside the launch (round 4): the queries are packed to two bits per symbol,
 * bucket-ordered on the device by the top 22 key bits (MSBWT_ORDER_BITS) in two passes, counted in index order, and every count
 * is returned to its query's own place in the caller's buffer -- the caller sees its order.  It is a SWITCH, off unless asked for:
 * mode 1 = whenever the passes apply (pair index, 12 <= k <= 64, 4096 <= n < 2^32); 0 = never; -1 = the default, which is never
 * too (kept as a value so that callers written against round 4 keep working).  There is no automatic mode: ordering 10^8 queries
 * and un-ordering their counts costs about 6 ms of the 8 ms the ordered search saved on the densest batches of round 4, sparse or
 * random batches lost 30 % to 2.7x -- and since round 5 the default index looks its queries up in a HASHED sparse suffix table,
 * whose lookups an order cannot help: the same dense batches now LOSE 6-14 % with the pass forced on (round 5, `library_ordered` beside
 * the c4_* lines of bench.py: 7.5 -> 6.8 and 7.9 -> 7.4 x 10^9 q/s).  MSBWT_ORDER=0|1 in the environment sets the initial mode.
 * Applies to msbwt_rle_count_kmers[_device] and the packed forms (not to the k-mer range and extension calls).  msbwt_rle_batch_order_for: 1 if a batch of n k-symbol queries
 * would be ordered now.  Results never change. */
int msbwt_rle_set_batch_order(msbwt_rle *bwt, int mode);
int msbwt_rle_get_batch_order(const msbwt_rle *bwt);
int msbwt_rle_batch_order_for(const msbwt_rle *bwt, size_t k, size_t n);
int msbwt_rle_kmer_order_keys_device(const msbwt_rle *bwt, const void *d_kmers, size_t k, size_t n, void *d_out_keys, void *hip_stream);

/* ---- tuning / introspection (no reference counterpart) ---- */
/* Depth of the precomputed suffix table (the reference's stubbed kmer_cache,
 * src/msbwt_core.rs:133-146): ranges for every ACGT suffix of length `depth` are computed
 * on the device at load time and replace the first `depth` steps of each query.  0 turns it
 * off, a negative value restores the automatic choice (the deepest table the data warrants
 * within max(1 GiB, 2 x block bytes), at most 15), the maximum is 16 (64 GiB).  Takes effect
 * immediately if an index is loaded.  Results never change. */
int msbwt_rle_set_table_depth(msbwt_rle *bwt, int depth);
int msbwt_rle_get_table_depth(const msbwt_rle *bwt);
/* Packed suffix table: beside a pair index the finished table can be extended by TWO more levels
 * and stored as 128-byte lines of 30 entries (16-bit deltas; 4.27 bytes per entry instead of 16),
 * e.g. depth 17 in 73 GB for a 30x human BWT.  One line fetch per query as before, one search step
 * fewer -- and it is the widest-range step, the one that usually needs two lines.  mode 1 = on
 * (whenever a pair index exists), 0 = off, -1 = automatic (default: when the table depth itself is
 * automatic, 4^(depth+2) <= 256 x total symbols and the lines fit in half of the free HBM -- the flat
 * parent table is then built as deep as that packed table needs, up to 15 levels, and freed;
 * MSBWT_TABLE_PACKED=0/1 overrides).
 * msbwt_rle_get_table_depth reports the effective depth (flat depth + 2).  Lines whose deltas do not
 * fit 16 bits are marked ESCAPE and keep their ranges in a side array (msbwt_rle_set_table_side, below).  Results never change.
 * Beside a sparse suffix table (msbwt_rle_set_sparse_table, the default since round 5) the automatic direct table stays at packed
 * depth 15 at most: only queries shorter than the sparse table's depth still read it. */
int msbwt_rle_set_table_packed(msbwt_rle *bwt, int mode);
/* Escape lines of the packed table -- lines holding a range 2^16 or more wide, or further than that from the line's
 * first range: the suffixes of high-copy repeats (Alu-, L1-like families, satellites) -- keep their 30 ranges as flat
 * 16-byte entries in a SIDE array (512 bytes per such line): a query that lands on one pays one more line fetch, like any
 * search step, instead of searching from scratch (the reference's constrain_range costs the same for any range width,
 * src/rle_bwt.rs:202-287).  mode 1 = on (default), 0 = off (MSBWT_TABLE_SIDE=0 in the environment).  Results never change.
 * msbwt_rle_table_info: lines of the packed table in HBM, how many are escape lines, bytes of the side array (all 0
 * without a packed table). */
int msbwt_rle_set_table_side(msbwt_rle *bwt, int mode);
int msbwt_rle_table_info(const msbwt_rle *bwt, uint64_t *lines, uint64_t *escape_lines, uint64_t *side_bytes);
/* The automatic choice, as a pure function (no device needed): levels of the flat table built first and of
 * the packed table it becomes (0 = stays flat), for an index of `total_symbols` symbols with `free_hbm_bytes`
 * of HBM free once plane and pair blocks are in place. */
int msbwt_auto_table_depths(uint64_t total_symbols, uint64_t free_hbm_bytes, int pair_index, int *flat_depth, int *packed_depth);
int msbwt_rle_get_table_packed(const msbwt_rle *bwt);
/* Sparse suffix table (the reference's stubbed kmer_cache, src/msbwt_core.rs:133-146 / src/rle_bwt.rs:332-346, taken past what a
 * direct-address table can hold): the ranges of the `depth`-symbol suffixes that OCCUR in the BWT, 16 <= depth <= 31, as a hashed
 * table of 128-byte buckets of 14 entries (12 with 32-bit tags from depth 25 on, 11 with 40-bit tags from depth 30 on; layout and hash: rust-msbwt_amd/csrc/sparse_table.hpp).  The direct table above has 4^depth
 * entries whatever the data -- 73 GB at depth 17, of which a 30x human read set can fill 17 % and a chr20-sized one 0.4 % -- while a
 * table of the present suffixes reaches depth 23 in about 14 bytes per distinct 23-mer: every present 31-mer is three pair steps
 * (of seven) shorter.  One lookup = one random 128-byte line, fetched like any search step's; the table is complete, so a miss is
 * count 0 (the early exit of src/msbwt_core.rs:151-153); entries 255 or more wide (suffixes of high-copy repeats) keep their range
 * in a side array, one more line.  Built on the device by frontier expansion with the index's own rank code (each present d-mer ->
 * its <= 16 present (d+2)-mers by one pair step), which also yields the DISTINCT counts per depth that size it.  Needs the pair
 * index; the one-query-per-lane kernel uses it for every batch with k >= depth, shorter k-mers (and k-mers with '$' / 'N' among
 * their last `depth` symbols) use the direct table, which then stays small (packed depth 15 at most when automatic).
 * depth: -1 = automatic (default: the deepest depth <= 23 whose table fits HBM -- and a memory budget, if one is set -- with an
 * eighth of the device left free; none if no depth fits, e.g. a read set whose error k-mers outnumber everything), 0 = off, 16..31 =
 * exactly that depth (an error if it cannot be built; a table serves k >= its depth: a caller that counts 31-mers gains two pair
 * steps per query from depth 27 -- 3 index lines instead of 5 -- and loses the table for k = 23..26).  MSBWT_SPARSE_TABLE=<depth>|auto|0 in the environment sets the initial mode.
 * Takes effect immediately if an index is loaded.  Results never change.
 * msbwt_rle_get_sparse_table: depth of the table in HBM, 0 = none.
 * msbwt_rle_sparse_table_info: out[MSBWT_SPARSE_INFO_WORDS] = [0] depth, [1] entries, [2] buckets, [3] bytes of the bucket lines,
 * [4] entries in the side array, [5] its bytes, [6] entries displaced to a later bucket, [7] depth of the direct table the build
 * started from, [9] buckets a lookup may go beyond its own, [10 + d] DISTINCT d-symbol suffixes that occur (d = 0..31; 0 where the
 * build did not pass: it advances two symbols at a time), [45 + d] of which 255 or more wide, [80 + d] of which exactly 1 wide (suffixes
 * that occur once: on reads with errors, mostly error k-mers), [8] 1 = the table is of the two-tier form, [42] suffixes in its filters,
 * [43] depth of the SECOND, shallower level (0 = none), [44] its bytes and [112] 1 = it is of the two-tier form: with k undeclared the table is 23 deep and serves k >= 23; where
 * the deep direct table of an index without a sparse table (packed depth 17) does not fit beside it but a table of the 17-symbol suffixes
 * does, that one is built as well and serves 17 <= k < 23 (MSBWT_SPARSE_SECOND=0: never), so that no k loses to the index without a
 * sparse table.
 * [113] / [114] / [115] chunks, retries and descents of the sizing pass's frontier walk, [116] / [117] / [118] of the last fill pass's
 * (as msbwt_rle_spectrum_info reports them for a spectrum walk; MSBWT_SPARSE_FRONTIER=<nodes> in the environment caps the builder's
 * frontier buffers, 64 nodes at least: tests).
 * The counts are kept even when no table was built.
 * TWO-TIER form (msbwt_rle_set_sparse_tiers; rust-msbwt_amd/csrc/sparse_table.hpp): the complete table's size follows the distinct
 * suffixes, and on reads WITH errors most of those occur once (a 30x human read set with 0.5 % substitutions: 1.3e10 distinct 23-mers,
 * 185 GB, of which about 3e9 -- the genome's -- occur more than once).  The two-tier table keeps entries only for the suffixes whose
 * range is at least 2 wide and sets, for each of the others, four bits of a filter inside its own bucket line (no false negatives):
 * a lookup that finds its tag is served as before, one that finds neither tag nor filter bits is count 0, and one whose filter bits are
 * set continues through the direct table and the search -- the reference's own path (src/rle_bwt.rs:202-287) -- so every count stays
 * exact whatever the filter says.  A two-tier level is always deeper than the direct table (its depth once packed): where it would not be,
 * that depth gets the complete table -- or, when both depths were set explicitly and mode is 1, the setter or load fails with
 * MSBWT_ERR_INVALID_ARG.  mode: -1 = automatic (default: the two-tier form of a depth where its complete table does not fit
 * HBM or the memory budget -- tried before the next shallower depth), 0 = complete tables only, 1 = two-tier only (tests, measurements).
 * MSBWT_SPARSE_TIERS=auto|0|1 sets the initial mode.  Takes effect immediately if an index is loaded.  Results never change.
 * msbwt_rle_get_sparse_tiers: 1 when the table in HBM is of the two-tier form, else 0.
 * msbwt_sparse_hash / msbwt_sparse_table_shape: the table's hash and sizing as pure functions (no device needed).
 * msbwt_rle_download_sparse_table: copies the bucket lines (and the side array) to the host; returns the bytes of the lines,
 * SIZE_MAX without a table or on error (tests check every entry against the oracle). */
#define MSBWT_SPARSE_INFO_WORDS 120
int msbwt_rle_set_sparse_table(msbwt_rle *bwt, int depth);
int msbwt_rle_get_sparse_table(const msbwt_rle *bwt);
int msbwt_rle_set_sparse_tiers(msbwt_rle *bwt, int mode);
int msbwt_rle_get_sparse_tiers(const msbwt_rle *bwt);
/* The second, shallower sparse level ([43] / [44] of msbwt_rle_sparse_table_info): -1 = automatic (default: k undeclared, plane blocks, the
 * deep direct table does not fit beside the sparse table but a table of the 17-symbol suffixes does), 0 = never.  MSBWT_SPARSE_SECOND=0|auto
 * sets the initial mode.  Takes effect immediately if an index is loaded.  Results never change. */
int msbwt_rle_set_sparse_second(msbwt_rle *bwt, int mode);
int msbwt_rle_sparse_table_info(const msbwt_rle *bwt, uint64_t *out);
int msbwt_sparse_hash(uint64_t key, int depth, uint64_t nbuckets, uint32_t *bucket, uint32_t *tag);
int msbwt_sparse_hash64(uint64_t key, int depth, uint64_t nbuckets, uint32_t *bucket, uint64_t *tag); /* the whole tag: 24, 32 or 40 bits by depth */
int msbwt_sparse_table_shape(int depth, uint64_t entries, uint64_t *nbuckets, int *probe);
/* The automatic depth as a pure function (no device needed; rust-msbwt_amd/csrc/sparse_policy.hpp): distinct[d] / wide[d] for d = 0..31
 * as msbwt_rle_sparse_table_info reports them ([10 + d], [45 + d]), the depth of the direct table the count started from, and the bytes
 * the table and its build scratch may take -> the depth the loader would build (0 = none fits) and the bytes of that table. */
int msbwt_auto_sparse_depth(const uint64_t *distinct, const uint64_t *wide, int parent_depth, uint64_t avail_bytes, int query_length, int *depth, uint64_t *table_bytes);
/* ... with the two-tier form in the choice: singles[d] as [80 + d] above, tiers as msbwt_rle_set_sparse_tiers -> also *two_tier (0 / 1). */
int msbwt_auto_sparse_choice(const uint64_t *distinct, const uint64_t *wide, const uint64_t *singles, int parent_depth, uint64_t avail_bytes, int query_length,
                             int tiers, int *depth, int *two_tier, uint64_t *table_bytes);
/* The two-tier filter as a pure function: the filter word (0..7, i.e. word 23 + that of the bucket line) and the four bits of a key with this tag. */
int msbwt_sparse_filter_bits(uint64_t tag, uint32_t *word, uint32_t *mask);
/* The k the index will mostly be asked about (0 = unknown, the default; MSBWT_QUERY_K in the environment sets the initial value).  The
 * reference's count_kmer takes any k per call and so does this library -- results never depend on the hint -- but a hashed table of
 * d-mers serves k >= d only, and every two symbols of depth save a present k-mer one index line: with k unknown the automatic sparse
 * table stops at depth 23 (every k >= 23 is served: 5 lines for a present 31-mer); a caller that declares k = 31 gets depth 31 -- the table's range IS the count, one line per query
 * (depth 29: 2 lines, 1.92e10 present 31-mers/s at 30x-human scale; depth 27: 3 lines, 1.34e10; k unknown: 5 lines, 8.4e9) -- and k = 21 gets depth 21.  Shorter k-mers than the table's depth use the
 * direct table as before.  Only the AUTOMATIC depth follows the hint (msbwt_rle_set_sparse_table(-1)); it takes effect immediately if an
 * index is loaded (the tables are rebuilt).  msbwt_auto_sparse_max_depth: the rule as a pure function. */
int msbwt_rle_set_query_length(msbwt_rle *bwt, int k);
int msbwt_rle_get_query_length(const msbwt_rle *bwt);
int msbwt_auto_sparse_max_depth(int query_length);
size_t msbwt_rle_download_sparse_table(const msbwt_rle *bwt, void *out_lines, size_t cap_bytes, void *out_side, size_t cap_side_bytes);
/* Presence filter: one bit per ACGT suffix of length min(12, table depth), set when some table
 * entry with that suffix is a non-empty range; at most 2 MiB, so it lives in L2 and decides
 * absent k-mers (random queries, small genomes) without fetching the table line.  Built on the
 * device from the table; dropped automatically when more than 90 % of its bits are set (it
 * could reject almost nothing).  mode 0 = off, otherwise automatic (MSBWT_FILTER=0 in the
 * environment turns it off).  get returns the filter depth, 0 if none.  Results never change. */
int msbwt_rle_set_presence_filter(msbwt_rle *bwt, int mode);
int msbwt_rle_get_presence_filter(const msbwt_rle *bwt);
/* Pair index: a second block array (1 byte per symbol) that stores, next to each BWT symbol,
 * the symbol one LF step further, so that one search step consumes TWO k-mer symbols for one
 * line fetch per bound (maths: rust-msbwt_amd/csrc/rank_ops.hpp).  Built on the device from
 * the loaded index.  mode 1 = on, 0 = off, -1 = on when it fits in half of the free HBM
 * (default; MSBWT_PAIR_INDEX=0/1 in the environment overrides).  Results never change. */
int msbwt_rle_set_pair_index(msbwt_rle *bwt, int mode);
int msbwt_rle_get_pair_index(const msbwt_rle *bwt);
/* Spacing of the pair blocks: 128 = disjoint blocks (1 byte per symbol); 96 = overlapping blocks that
 * also hold the first 32 positions of their successor (1.33 bytes per symbol), so that a range up to
 * 32 wide is ranked from ONE line -- on real 30x data ranges stay ~25 wide to the last step and every
 * fifth step would otherwise fetch a second line.  0 = automatic (default; MSBWT_PAIR_STRIDE=96|128
 * overrides): 96 when that takes at most a quarter of the free HBM; otherwise the DATA decide -- at load time a
 * few thousand present 24-mers are read off the index by LF walks and counted, and overlapping blocks are built
 * when their median count (msbwt_rle_get_typical_range_width) is >= 8 and the bigger blocks fit beside the
 * suffix table with an eighth of the HBM to spare.  get returns 0 without a pair index.  Results never change. */
int msbwt_rle_set_pair_stride(msbwt_rle *bwt, int stride);
int msbwt_rle_get_pair_stride(const msbwt_rle *bwt);
/* Median number of occurrences of a 24-mer that is present in the index (4096 LF walks from pseudo-random rows,
 * probed once per load): about the coverage on a real read set, 1 on a stream of independent symbols; the width
 * the ranges of surviving queries keep through the search.  -1 = not probed (run blocks, empty index). */
double msbwt_rle_get_typical_range_width(const msbwt_rle *bwt);
/* The automatic spacing as a pure function (no device needed): for an index of `total_symbols` symbols with
 * `free_hbm_bytes` free once the plane blocks are in place on a device of `hbm_total_bytes`, given the typical
 * range width the probe reports (negative = unknown). */
int msbwt_auto_pair_stride(uint64_t total_symbols, uint64_t free_hbm_bytes, uint64_t hbm_total_bytes, double typical_width, int *stride);
/* A memory budget for the whole index -- the analogue of the reference's one space / time knob, `bin_power`
 * (src/rle_bwt.rs:309-322; here results never depend on it, only speed).  bytes = HBM the loaded index may hold, 0 = no budget
 * (default; MSBWT_MEMORY_BUDGET=<bytes> in the environment sets the initial value).  The plane blocks (0.5 byte per symbol) are
 * always built; what the budget leaves goes, in this order, to the pair blocks (whenever they fit), to the
 * deepest packed suffix table that fits, and to overlapping pair blocks when the data keep ranges wide -- one plan, made
 * at load time (or at once, if an index is loaded: the optional structures are rebuilt).  Explicit settings
 * (msbwt_rle_set_table_depth, _set_pair_index, _set_pair_stride, an explicit _set_sparse_table depth) still win over the plan.
 * The sparse suffix table takes what the budget leaves once blocks, pair blocks and a direct table of packed depth 15 are paid for
 * (the deepest depth that fits; none if nothing does -- the direct table is then as deep as the plan says).  Not counted against
 * the budget: the presence filter (2 MiB at most) and the side arrays of the tables (bytes per high-copy suffix).  A budget below
 * the plane blocks cannot be met -- they are built all the same -- and run blocks have no optional structure to plan: both are
 * said by msbwt_rle_last_error after the call, which still returns MSBWT_OK.
 * msbwt_auto_index_plan: the plan as a pure function (no device needed) for an index of `total_symbols` symbols with
 * `free_hbm_bytes` free once its plane blocks are in place; *index_bytes (optional) = what the planned index holds
 * (presence filter, at most 2 MiB, and the table's side array not counted). */
int msbwt_rle_set_memory_budget(msbwt_rle *bwt, uint64_t bytes);
uint64_t msbwt_rle_get_memory_budget(const msbwt_rle *bwt);
int msbwt_auto_index_plan(uint64_t total_symbols, uint64_t free_hbm_bytes, uint64_t hbm_total_bytes, double typical_width, uint64_t budget_bytes,
                          int *pair_index, int *pair_stride, int *flat_depth, int *packed_depth, uint64_t *index_bytes);
/* Block format of the index, chosen BEFORE a load (MSBWT_BLOCKS=runs in the environment sets the
 * initial choice): 0 = bit-plane blocks (default: 0.5 byte per symbol, fastest, the only format the
 * pair index, the packed table and the batch-ordering pass work on), 1 = run blocks -- the layout of the
 * reference's run_block_av_flat (src/run_block_av_flat.rs:43-56,97-125): 128-byte blocks of 512 positions
 * with per-block counts and 96 one-byte runs, ~0.3 byte per symbol on 30x short-read BWTs, single-symbol
 * steps only (no pair index).  Built on the device from the RLE bytes like the default format; for
 * 6 <= k <= 64 the lane-per-query kernel serves it too (each lane decodes its own block's runs from LDS):
 * a 30x human-scale BWT in 44 GB at 1.8 x 10^9 present 31-mers/s (bit planes + pair blocks + table:
 * 238 GB, 5.4 x 10^9).  For replicas that must leave HBM to others.  Results never change. */
/* msbwt_run_build_fits_device (pure, no device needed): 1 when the DEVICE builder of the run-block format fits `free_hbm_bytes` of free
 * HBM for an index of that many symbols -- it holds the plane blocks (0.5 byte per symbol) beside the run blocks (~0.3) for a moment;
 * when it does not (or an allocation fails on the way) the load builds the run blocks on the host and uploads them, as MSBWT_BUILD=host
 * always does: an index that fits only BECAUSE the format is lean still loads. */
int msbwt_run_build_fits_device(uint64_t total_symbols, uint64_t free_hbm_bytes);
int msbwt_rle_set_block_format(msbwt_rle *bwt, int format);
int msbwt_rle_get_block_format(const msbwt_rle *bwt);
/* Search kernel for 1 <= k <= 64: 0 = automatic (default: 2 whenever a pair index exists and k >= 6, and on run
 * blocks for k >= 6), 1 = 8 lanes per query, lines in registers (kernels.hip; one symbol per step; needs no pair index),
 * 2 = one query per lane, lines staged through LDS by LDS-DMA (lanes.hip; two symbols per step,
 * 8x more random lines in flight per wave).  MSBWT_SEARCH=groups|lanes in the environment
 * sets the initial mode.  Results never change. */
int msbwt_rle_set_search_kernel(msbwt_rle *bwt, int mode);
int msbwt_rle_get_search_kernel(const msbwt_rle *bwt);
/* The kernel a batch of k-symbol queries runs on with the index and mode as they are now: 1 or 2 as
 * above, 0 for k > 64 (generic 8-lane kernel, no suffix table); negative = error. */
int msbwt_rle_search_kernel_for(const msbwt_rle *bwt, size_t k);
/* Search counters (measurement aid, off by default): with them on, every wave of the one-query-per-lane kernel adds what its
 * queries did to a block of MSBWT_SEARCH_COUNTERS u64 -- [0] search steps of a wave, [1] steps taken by a query (one line
 * fetch each), [2] of which two-symbol steps, [3] steps that needed a second line (range over two blocks), [4] steps a query
 * waited because the second-line slots of its wave were taken, [5] queries whose packed-table line is an escape line,
 * [6] of which searched from scratch (no side array), [7] queries decided by the table / presence filter alone, [8] queries
 * that entered the search, [9] first lines fetched, [10] sparse-table bucket lines fetched (included in [1]), [11] of which did not
 * hold the key although the bucket had displaced entries (the lookup went on to the next bucket), [12] of [10], lookups that rode
 * along with the search of the tile before theirs (in second-line slots that step left free) instead of taking a step of their own, [13] waves of the
 * persistent kernel that were dealt at least one tile; the rest 0.  msbwt_rle_search_counters copies the block out and
 * zeroes it (synchronises `hip_stream`, on which the counted launches ran).  Results never change. */
#define MSBWT_SEARCH_COUNTERS 16
int msbwt_rle_set_search_counters(msbwt_rle *bwt, int enabled);
int msbwt_rle_search_counters(const msbwt_rle *bwt, uint64_t *out, void *hip_stream);
/* Cache policy of the index lines.  The one-query-per-lane kernel uses every line it fetches once; on an index whose random-access
 * arrays (the pair blocks, else the blocks themselves) are far larger than L2 and the 256 MB Infinity Cache those lines only evict what
 * IS reused (the superblock table, the query stream), so they are fetched with the non-temporal hint: at 30x-human scale 36.1 ms per
 * 3 x 10^8 present 31-mers (35.6-36.6 over four alternating runs) against 38.4 ms (36.7-39.8) with the default policy; a small index,
 * whose pair blocks half live in the Infinity Cache, LOSES (C3 fused 14.9 -> 19.8 ms).  mode -1 = automatic (default: from 4 GiB of such
 * arrays on), 0 = never, 1 = always; MSBWT_STREAM_LINES=0|1|auto in the environment sets the initial mode.  get: what launches on the
 * loaded index do now.  Results never change. */
int msbwt_rle_set_line_streaming(msbwt_rle *bwt, int mode);
int msbwt_rle_get_line_streaming(const msbwt_rle *bwt);
/* Placement diagnostic: random 128-byte lines per second the memory system serves right now from one of the index's arrays
 * (which: 0 = plane / run blocks, 1 = pair blocks, 2 = the sparse table's bucket lines, 3 = the direct suffix table; 0.0 when the
 * index has no such array) -- about a millisecond of gathering, nothing is written.  (Round 5 used it on the "two modes" of C4-sized
 * indexes -- the same launch 12 or 14 ms per instance of the index: a plain gather does not see them, profiles/r05_lab/two_modes.log.) */
int msbwt_rle_probe_line_rate(const msbwt_rle *bwt, int which, double *lines_per_second);
/* Bytes of HBM held by the index (blocks + table + filter + pair index). */
uint64_t msbwt_rle_device_bytes(const msbwt_rle *bwt);
/* Average duration in ms of the count kernel launches since the last reset, measured with
 * HIP events on the launch stream (bench.py's roofline uses it); resets the accumulator. */
int msbwt_rle_kernel_time_ms(const msbwt_rle *bwt, double *avg_ms, uint64_t *launches);
int msbwt_rle_set_kernel_timing(msbwt_rle *bwt, int enabled);
int msbwt_rle_device_ordinal(const msbwt_rle *bwt);
const char *msbwt_rle_last_error(const msbwt_rle *bwt);
/* Host half of the load path, exposed for inspection (no device needed): expands an RLE
 * stream into the plane blocks the kernels read (layout: rust-msbwt_amd/csrc/plane_index.hpp).
 * Returns the number of 128-byte blocks (= total/256 + 1); writes at most `cap_blocks` of
 * them to out_blocks (may be NULL), the symbol total to *out_total. SIZE_MAX on bad input. */
size_t msbwt_build_plane_blocks(const uint8_t *rle_bytes, size_t len, void *out_blocks, size_t cap_blocks,
                                uint64_t *out_total);
/* The same for the run-block format (layout: rust-msbwt_amd/csrc/run_index.hpp): returns the number
 * of 128-byte blocks (= total/512 + 1); out_overflow receives 256 bytes per overflowing block
 * (*out_noverflow of them).  Call with NULL outputs to size.  SIZE_MAX on bad input. */
size_t msbwt_build_run_blocks(const uint8_t *rle_bytes, size_t len, void *out_blocks, size_t cap_blocks,
                              void *out_overflow, size_t cap_overflow, uint64_t *out_total, uint64_t *out_noverflow);
/* Copies the index as it sits in HBM back to the host (same layout as
 * msbwt_build_plane_blocks); returns the block count, SIZE_MAX on error.  Lets tests compare
 * the device-side builder with the host one. */
size_t msbwt_rle_download_blocks(const msbwt_rle *bwt, void *out_blocks, size_t cap_blocks);
const char *msbwt_version(void);

/* ---- codecs either side of the path ---- */
/* convert_to_vec (src/bwt_converter.rs:26-80): ASCII "$ACGNT" (+ '\n', ignored) -> RLE
 * bytes.  Returns the number of bytes needed/written; out may be NULL to size.  Returns
 * SIZE_MAX for a byte outside the alphabet (the reference panics). */
size_t msbwt_convert_to_vec(const uint8_t *ascii, size_t n, uint8_t *out, size_t cap);
/* save_bwt_numpy (src/bwt_converter.rs:102-130): 96-byte NumPy v1.0 header + payload */
int msbwt_save_bwt_numpy(const uint8_t *rle_bytes, size_t n, const char *utf8_path);
/* save_bwt_runs_numpy (src/bwt_converter.rs:151-184) */
int msbwt_save_bwt_runs_numpy(const uint8_t *syms, const uint64_t *counts, size_t nruns,
                              const char *utf8_path);
/* string_util (src/string_util.rs:3-88) */
void msbwt_convert_stoi(const uint8_t *ascii, size_t n, uint8_t *out_codes);
void msbwt_convert_itos(const uint8_t *codes, size_t n, uint8_t *out_ascii);
void msbwt_reverse_complement_i(const uint8_t *codes, size_t n, uint8_t *out_codes);

#ifdef __cplusplus
}
#endif
#endif
