/*
 * include/adl_bloom.h -- C-ABI of the MI355X (gfx950) SSTable bloom-filter
 * build/probe layer (libadlbloom.so).
 *
 * This is the drop-in boundary for the reference's filter path
 * (adlternative/adlsm-tree):
 *   - src/murmur3_hash.hpp:9        uint32_t murmur3_hash(seed, data, len)
 *   - src/filter_block.hpp:22-34    class BloomFilter : FilterAlgorithm
 *       Keys2Block(const vector<string>&, string&)   (src/filter_block.cpp:9-33)
 *       IsKeyExists(string_view key, string_view bm) (src/filter_block.cpp:49-62)
 *   - src/filter_block.hpp:36-73    FilterBlockWriter / FilterBlockReader
 * The host C++ mirror of those classes (adlsm-tree_amd/csrc/filter_block.hpp)
 * and any FFI binding (ctypes) call only what is declared
 * here: plain pointers and sizes, no C++ or torch types, no exceptions.
 *
 * Key sets are packed: `keys` is a byte buffer; key i is
 *   keys[offsets[i] .. offsets[i+1])          when offsets != NULL (n+1 entries)
 *   keys[i*key_stride .. (i+1)*key_stride)    when offsets == NULL
 * Bitmaps are the reference's bytes exactly: n*bits_per_key + 7 bytes, bit b
 * of the filter is bit (b & 7) of byte (b >> 3).
 *
 * Every function returns an adl_status (0 = OK).  All entry points are
 * re-entrant and thread-safe: work is enqueued on the caller's HIP stream
 * (`stream`, a hipStream_t) and nothing global is mutated after the
 * once-guarded device query.  Functions named *_device take device pointers
 * and do not synchronise; there NULL = the null stream.  The others take host
 * pointers and return when the results are in host memory; there NULL = a
 * non-blocking stream of the calling thread (created on first use), so calls
 * from different threads run side by side on the device instead of queueing
 * on the legacy null stream.
 */
#ifndef ADL_BLOOM_H_
#define ADL_BLOOM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADL_BLOOM_ABI_VERSION 1

/* Status codes.  ADL_OK and ADL_FILTER_BLOCK_ERROR keep the values of the
 * reference's enum RC (src/rc.hpp:8-39: OK = 0, FILTER_BLOCK_ERROR = 13); the
 * negative codes are device/argument failures the CPU reference cannot have. */
typedef enum adl_status {
  ADL_OK = 0,
  ADL_FILTER_BLOCK_ERROR = 13, /* malformed filter block (src/filter_block.cpp:113-170) */
  ADL_ERR_INVALID_ARG = -1,    /* NULL pointer, negative bits_per_key, bad offsets/alignment */
  ADL_ERR_TOO_LARGE = -2,      /* n*bits_per_key+7 exceeds the reference's int range */
  ADL_ERR_DEVICE = -3,         /* HIP runtime / launch failure, no GPU */
  ADL_ERR_OUT_OF_MEMORY = -4,  /* device allocation failed */
  ADL_ERR_WORKSPACE = -5       /* caller workspace smaller than required */
} adl_status;

/* Human-readable text for a status (static storage). */
const char *adl_bloom_strerror(int status);

/* ABI version of the loaded library (== ADL_BLOOM_ABI_VERSION). */
int adl_bloom_abi_version(void);

/* k = (int)(bits_per_key * 0.69) clamped to [1, 30]  (src/filter_block.cpp:44-46). */
int32_t adl_bloom_num_probes(int32_t bits_per_key);

/* Bitmap size in bytes, n*bits_per_key + 7 (src/filter_block.cpp:11-14); 0 when
 * the reference's `int` arithmetic would overflow or bits_per_key < 0. */
uint64_t adl_bloom_bitmap_bytes(uint64_t n, int32_t bits_per_key);

/* Device buffer size a *_device build writes for one filter: the bitmap rounded
 * up to 16 bytes (the pad bytes are written as zero). */
uint64_t adl_bloom_bitmap_alloc_bytes(uint64_t n, int32_t bits_per_key);

/* ---------------------------------------------------------------- build */

/* Workspace (device bytes) adl_bloom_build_device / _segmented_device need for
 * filters with the given key counts (num_filters entries).  key_counts is a
 * HOST array. */
uint64_t adl_bloom_build_workspace_bytes(const uint64_t *key_counts, uint32_t num_filters,
                                         int32_t bits_per_key);

/* Build one filter from device-resident keys into a device bitmap.
 * Replaces BloomFilter::Keys2Block (src/filter_block.cpp:9-33) for a batch.
 *   d_bitmap: adl_bloom_bitmap_alloc_bytes(n, bpk) bytes, 16-byte aligned;
 *             every byte is written (no pre-zeroing needed).
 *   d_workspace: adl_bloom_build_workspace_bytes(&n, 1, bpk) bytes, 256-B aligned.
 *   d_keys: no alignment or padding is required.  When it is 16-byte aligned
 *   the kernels may load whole aligned 16-byte blocks that hold key bytes, so
 *   up to 15 bytes past the last key's end are read (never a block that holds
 *   no key byte, so never a page the keys do not touch); when it is not, every
 *   access stays inside the key bytes. */
int adl_bloom_build_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                           uint32_t key_stride, int32_t bits_per_key, uint8_t *d_bitmap,
                           void *d_workspace, uint64_t workspace_bytes, void *stream);

/* Build num_filters independent filters (one per SSTable) in one pass pair
 * (split only past 2^31 / k keys, where u32 position indices would overflow).
 * Filter f owns keys [key_begin[f], key_begin[f+1]) of the key set and writes
 * its bitmap at d_bitmaps + bitmap_off[f] (16-byte aligned, room for
 * adl_bloom_bitmap_alloc_bytes(n_f, bpk)).  key_begin (num_filters+1 entries)
 * and bitmap_off (num_filters entries) are HOST arrays. */
int adl_bloom_build_segmented_device(const uint8_t *d_keys, const uint64_t *d_offsets,
                                     uint32_t key_stride, const uint64_t *key_begin,
                                     uint32_t num_filters, int32_t bits_per_key,
                                     uint8_t *d_bitmaps, const uint64_t *bitmap_off,
                                     void *d_workspace, uint64_t workspace_bytes, void *stream);

/* Flags for adl_bloom_build_segmented_device_ex. */
#define ADL_BLOOM_SKIP_ADJACENT_DUPLICATES 1u /* a key equal to the previous key of its
  filter is not hashed: same bitmap (OR is idempotent, and m still counts every key
  as Keys2Block's keys.size() does), less work when versions of one user key arrive
  in a row (memtable order, src/keys.cpp:61-74; SSTableWriter::Add, src/sstable.cpp:28) */

/* adl_bloom_build_segmented_device with flags (0 = identical to it). */
int adl_bloom_build_segmented_device_ex(const uint8_t *d_keys, const uint64_t *d_offsets,
                                        uint32_t key_stride, const uint64_t *key_begin,
                                        uint32_t num_filters, int32_t bits_per_key,
                                        uint8_t *d_bitmaps, const uint64_t *bitmap_off, uint32_t flags,
                                        void *d_workspace, uint64_t workspace_bytes, void *stream);

/* Host-pointer convenience: upload keys, build, download exactly
 * adl_bloom_bitmap_bytes(n, bpk) bytes into h_bitmap (which may be unaligned,
 * e.g. the tail of a std::string as in Keys2Block).  Synchronous.  The same
 * path as adl_bloom_build_segmented with one filter: pinned (hipHostMalloc'd /
 * registered) key and bitmap buffers are DMAed directly, pageable ones staged
 * through per-thread pinned buffers.  Replaces BloomFilter::Keys2Block
 * (src/filter_block.cpp:9-33). */
int adl_bloom_build(const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t n,
                    uint32_t key_stride, int32_t bits_per_key, uint8_t *h_bitmap,
                    void *stream);

/* Host-pointer segmented build for many filters (the compaction shape: one
 * filter per SSTable, keys and bitmaps in host memory), pipelined: filters go
 * in groups (~128 MB of keys, one launch pair each) whose key upload, build
 * (on `stream`) and bitmap download overlap on three streams.  Filter f's bitmap,
 * exactly adl_bloom_bitmap_bytes(n_f, bpk) bytes, is written at
 * h_bitmaps + h_bitmap_off[f] (any alignment, e.g. packed back to back as in
 * a filter block).  Pinned (hipHostMalloc'd / registered) buffers are DMAed
 * directly; pageable ones are staged through per-thread pinned buffers.
 * key_begin (num_filters+1) and h_bitmap_off (num_filters) are HOST arrays.
 * Synchronous.  Replaces num_filters calls of BloomFilter::Keys2Block
 * (src/filter_block.cpp:9-33) from SSTableWriter::Final (src/sstable.cpp:58). */
int adl_bloom_build_segmented(const uint8_t *h_keys, const uint64_t *h_offsets, uint32_t key_stride,
                              const uint64_t *key_begin, uint32_t num_filters, int32_t bits_per_key,
                              uint8_t *h_bitmaps, const uint64_t *h_bitmap_off, void *stream);

/* adl_bloom_build_segmented with flags (ADL_BLOOM_SKIP_ADJACENT_DUPLICATES; 0 =
 * identical to it): the host side of SSTableWriter::Final (src/sstable.cpp:58),
 * whose filters hold the user keys of a memtable run, versions of one user key
 * in a row (src/sstable.cpp:28, src/keys.cpp:61-74). */
int adl_bloom_build_segmented_ex(const uint8_t *h_keys, const uint64_t *h_offsets, uint32_t key_stride,
                                 const uint64_t *key_begin, uint32_t num_filters, int32_t bits_per_key,
                                 uint8_t *h_bitmaps, const uint64_t *h_bitmap_off, uint32_t flags, void *stream);

/* --------------------------------------------------------- streamed build */

/* A filter builder that takes its keys in batches while a table fills
 * (SSTableWriter::Add -> FilterBlockWriter::Update, src/sstable.cpp:28,
 * src/filter_block.cpp:72-75) and builds at the end (FilterBlockWriter::Final,
 * src/filter_block.cpp:104-109, src/sstable.cpp:58).  Every appended key is
 * hashed on arrival; the object keeps the two murmur hashes of each key, 8
 * bytes, in one device array in key order, and the filter bounds on the host.
 * A finish builds every filter from those pairs: it uploads and hashes
 * nothing.  The bitmaps are those adl_bloom_build_segmented_device_ex gives
 * for the same keys and bounds, bit for bit.
 *
 * Not thread-safe: one thread at a time per object; different objects may be
 * used from different threads concurrently.  Buffers an object has outgrown
 * are released by a reset once its appends and finishes have completed, and
 * otherwise when it is destroyed. */
typedef struct adl_bloom_stream adl_bloom_stream;

/* Keys per workgroup of the append kernel for keys that are not aligned
 * 16-byte keys (tests place batch sizes around it). */
#define ADL_BLOOM_STREAM_RUN_KEYS 512

/* reserve_keys: pairs the first allocation has room for (a hint; the store
 * grows geometrically, the copy ordered on the growing append's stream).
 * Nothing is allocated before the first append. */
int adl_bloom_stream_create(uint64_t reserve_keys, adl_bloom_stream **stream_out);
/* Waits for the object's appends and finishes in flight. */
int adl_bloom_stream_destroy(adl_bloom_stream *s);
/* Empties the object (no keys, no filters) and keeps its capacity. */
int adl_bloom_stream_reset(adl_bloom_stream *s);

/* Append n HOST keys, (keys, offsets | stride) as in adl_bloom_build, to the
 * open filter.  The batch is copied into the calling thread's pinned staging;
 * its upload and hashing are enqueued on `stream` and the call returns without
 * waiting for the device (it waits only when the thread's staging slots are all
 * in flight).  h_keys / h_offsets may be reused on return.  n == 0: no-op.
 * Offsets that decrease: ADL_ERR_INVALID_ARG.  stream == NULL: the calling
 * thread's own non-blocking stream, as for the other host-pointer calls. */
int adl_bloom_stream_append(adl_bloom_stream *s, const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t n,
                            uint32_t key_stride, void *stream);

/* The same for a DEVICE-resident batch, under the build's read contract: a
 * 16-byte-aligned d_keys may be read up to 15 bytes past the batch's last key;
 * of any other d_keys no byte outside the batch's keys is read.  The batch
 * must stay untouched until the stream's work is done. */
int adl_bloom_stream_append_device(adl_bloom_stream *s, const uint8_t *d_keys, const uint64_t *d_offsets,
                                   uint64_t n, uint32_t key_stride, void *stream);

/* Close the open filter, as FilterBlockWriter::Keys2Block() does.  Cuts with
 * no key between them make empty filters. */
int adl_bloom_stream_cut(adl_bloom_stream *s);

/* The filters so far: *num_filters, and (key_begin != NULL) their bounds,
 * num_filters + 1 entries (capacity smaller: ADL_ERR_INVALID_ARG, with
 * *num_filters set).  Keys after the last cut count as a last filter, as
 * Final's implicit Keys2Block does. */
int adl_bloom_stream_counts(const adl_bloom_stream *s, uint32_t *num_filters, uint64_t *key_begin,
                            uint32_t capacity);

/* adl_bloom_build_workspace_bytes of the object's filters as they stand. */
uint64_t adl_bloom_stream_finish_workspace_bytes(const adl_bloom_stream *s, int32_t bits_per_key);

/* Build every filter of the object from its pairs: filter f's bitmap goes to
 * d_bitmaps + bitmap_off[f] (HOST array, one entry per filter of
 * adl_bloom_stream_counts).  Bitmaps, workspace, flags
 * (ADL_BLOOM_SKIP_ADJACENT_DUPLICATES: a key whose pair equals its
 * predecessor's is skipped, the same bitmap), launch-group split and statuses
 * are those of adl_bloom_build_segmented_device_ex; an object without a filter
 * is ADL_ERR_INVALID_ARG, a short workspace ADL_ERR_WORKSPACE with nothing
 * enqueued.  Enqueued on `stream` behind every earlier append of the object,
 * whatever stream that ran on.  The object is not consumed: it may be
 * appended to and finished again, also with another bits_per_key. */
int adl_bloom_stream_finish_device(adl_bloom_stream *s, int32_t bits_per_key, uint32_t flags, uint8_t *d_bitmaps,
                                   const uint64_t *bitmap_off, void *d_workspace, uint64_t workspace_bytes,
                                   void *stream);

/* The same into HOST memory: filter f's bitmap, exactly
 * adl_bloom_bitmap_bytes(n_f, bpk) bytes, at h_bitmaps + h_bitmap_off[f] (any
 * alignment), as adl_bloom_build_segmented_ex writes them.  Synchronous
 * (stream == NULL: the calling thread's own stream). */
int adl_bloom_stream_finish(adl_bloom_stream *s, int32_t bits_per_key, uint32_t flags, uint8_t *h_bitmaps,
                            const uint64_t *h_bitmap_off, void *stream);

/* ------------------------------------------------- filter block on the device */

/* Size of the filter block FilterBlockWriter::Final (src/filter_block.cpp:77-102)
 * writes for num_filters filters, filter f holding keys [key_begin[f],
 * key_begin[f+1]) (HOST array, num_filters+1 entries): the bitmaps back to back
 * (n_f*bpk+7 bytes each), then i32 offsets[F], i32 offsets_start, i32 F,
 * "bf:" + i32 bpk, i32 7.  0 on invalid input or a block beyond the
 * reference's int offsets. */
uint64_t adl_bloom_filter_block_bytes(const uint64_t *key_begin, uint32_t num_filters,
                                      int32_t bits_per_key);

/* Workspace for adl_bloom_filter_block_build_device: the build workspace plus
 * the 16-byte-aligned bitmaps before they are packed. */
uint64_t adl_bloom_filter_block_workspace_bytes(const uint64_t *key_begin, uint32_t num_filters,
                                                int32_t bits_per_key);

/* Build num_filters filters from device-resident keys and frame them as one
 * filter block in d_block (16-byte aligned, >= adl_bloom_filter_block_bytes):
 * byte-identical to FilterBlockWriter::Keys2Block() per filter followed by
 * Final() (src/filter_block.cpp:77-109), so one D2H -- or one direct file
 * write -- emits the block.  num_filters == 0 gives the 19-byte empty block. */
int adl_bloom_filter_block_build_device(const uint8_t *d_keys, const uint64_t *d_offsets,
                                        uint32_t key_stride, const uint64_t *key_begin,
                                        uint32_t num_filters, int32_t bits_per_key,
                                        uint8_t *d_block, uint64_t block_bytes, void *d_workspace,
                                        uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------- probe */

/* Probe n keys against one device bitmap of bitmap_bytes bytes (the exact
 * reference length; m = bitmap_bytes*8 as in src/filter_block.cpp:50).
 * d_out[i] = 1 if key i may be present, 0 if it is certainly absent.
 * Replaces BloomFilter::IsKeyExists (src/filter_block.cpp:49-62) for a batch. */
int adl_bloom_probe_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                           uint32_t key_stride, int32_t bits_per_key, const uint8_t *d_bitmap,
                           uint64_t bitmap_bytes, uint8_t *d_out, void *stream);

/* Probe n keys, key i against filter d_filter_id[i] of num_filters resident
 * bitmaps; filter f is d_bitmaps[d_bitmap_off[f] .. d_bitmap_off[f+1]) (device
 * array, num_filters+1 entries).  A filter id >= num_filters answers 0, as
 * FilterBlockReader::IsKeyExists does (src/filter_block.cpp:174). */
int adl_bloom_probe_multi_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                                 uint32_t key_stride, const uint32_t *d_filter_id,
                                 uint32_t num_filters, const uint8_t *d_bitmaps,
                                 const uint64_t *d_bitmap_off, int32_t bits_per_key,
                                 uint8_t *d_out, void *stream);

/* Like adl_bloom_probe_multi_device, with filter f = d_bitmaps[d_begin[f] ..
 * d_end[f]) (device arrays, num_filters entries each): the filters may sit
 * anywhere in one device arena, in any order (adl_bloom_filter_cache). */
int adl_bloom_probe_ranges_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                                  uint32_t key_stride, const uint32_t *d_filter_id,
                                  uint32_t num_filters, const uint8_t *d_bitmaps,
                                  const uint64_t *d_begin, const uint64_t *d_end,
                                  int32_t bits_per_key, uint8_t *d_out, void *stream);

/* Fan-out probe: key i against every filter of its own list, d_pair_filter
 * [d_pair_begin[i] .. d_pair_begin[i+1]) (device arrays: num_keys+1 u32 with
 * d_pair_begin[0] == 0, non-decreasing, d_pair_begin[num_keys] == num_pairs;
 * num_pairs filter ids).  d_out[p] (num_pairs bytes, pair order) is what
 * adl_bloom_probe_ranges_device answers for the pair (key i, d_pair_filter[p])
 * -- bit for bit, including 0 for a filter id >= num_filters, an empty filter
 * and one of 2^31 bits or more -- but each key is uploaded and hashed once
 * for all its filters.  d_end == NULL: filter f = d_bitmaps[d_begin[f] ..
 * d_begin[f+1]) (num_filters+1 entries).  num_keys == 0 or num_pairs == 0
 * launches nothing.  This is Level::Get's shape (src/revision.cpp:265-310: one
 * lookup key, every table of the level whose range covers it). */
int adl_bloom_probe_fanout_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t num_keys,
                                  uint32_t key_stride, const uint32_t *d_pair_begin,
                                  const uint32_t *d_pair_filter, uint64_t num_pairs, uint32_t num_filters,
                                  const uint8_t *d_bitmaps, const uint64_t *d_begin, const uint64_t *d_end,
                                  int32_t bits_per_key, uint8_t *d_out, void *stream);

/* Large-batch probe with a workspace: the answers of adl_bloom_probe_multi_device
 * (d_bitmap_end == NULL) or adl_bloom_probe_ranges_device (filter f =
 * d_bitmaps[d_bitmap_off[f] .. d_bitmap_end[f])).  For big batches over 1 to
 * 4096 filters (n < 2^31 - 1) it runs the tile-binned pipeline (queries
 * grouped by filter, positions sorted by 2^20-bit tile, bits tested in LDS:
 * streaming traffic instead of random bitmap reads); otherwise
 * the direct kernel.  The answers are the same bit for bit.  Which batches
 * take the pipeline:
 *   - 16-byte keys (d_offsets == NULL, key_stride == 16) at a 16-byte-aligned
 *     d_keys, from n = 2^20 on.  16-byte keys at an unaligned pointer stay on
 *     the direct kernel: the workspace size cannot depend on the pointer, and
 *     its answer for key_stride == 16 is the aligned plan's.
 *   - variable-length keys (d_offsets != NULL: n + 1 offsets from any base)
 *     and any other fixed stride, at any alignment, from
 *     ADL_BLOOM_PROBE_BATCH_VAR_MIN queries on (an environment switch, read
 *     again by adl_bloom_reload_knobs: 0 never, 1 .. 2^20 mean 2^20; not set:
 *     the measured crossover).  Their keys are hashed
 *     first, in runs of 512 staged in LDS and sorted by length, into n * 8
 *     more bytes of workspace.
 * adl_bloom_probe_batch_workspace_bytes takes key_stride == 0 for
 * variable-length keys (what a caller with d_offsets passes) and returns 256
 * for a batch that stays on the direct kernel.  A batch that takes the
 * pipeline with less workspace than its plan needs returns ADL_ERR_WORKSPACE.
 * The size is the largest plan of any k up to num_probes(bits_per_key): the
 * call's own plan wherever plans grow with k, and up to 1.1 % more where the
 * quantised chunk size makes a plan of many filters and few queries step down
 * (4096 filters, 2^20 queries); it never shrinks as k grows.
 * Read contract, as for every probe: d_keys at any alignment, and no byte
 * outside [d_keys + off(0), d_keys + off(n)) is read -- the hashing kernel
 * stages whole aligned 16-byte blocks only where they lie inside that range,
 * and reads the two blocks the range starts and ends in byte by byte.
 * A filter of 0 bytes or of 2^31 bits or more answers 0.  Replaces
 * BloomFilter::IsKeyExists (src/filter_block.cpp:49-62) over a multi-get
 * batch.  d_workspace: 256-byte aligned,
 * adl_bloom_probe_batch_workspace_bytes(n, num_filters, bpk, key_stride) bytes. */
uint64_t adl_bloom_probe_batch_workspace_bytes(uint64_t n, uint32_t num_filters, int32_t bits_per_key,
                                               uint32_t key_stride);
int adl_bloom_probe_batch_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n, uint32_t key_stride,
                                 const uint32_t *d_filter_id, uint32_t num_filters, const uint8_t *d_bitmaps,
                                 const uint64_t *d_bitmap_off, const uint64_t *d_bitmap_end, int32_t bits_per_key,
                                 uint8_t *d_out, void *d_workspace, uint64_t workspace_bytes, void *stream);

/* adl_bloom_probe_batch_device with a probe count per filter (filter blocks
 * written under different bits_per_key; the reference reads bpk per block,
 * src/filter_block.cpp:158-170).  The plan is made from max_k, which bounds
 * every filter's k: chunk size and entry regions are those of a uniform call
 * with k = max_k, and a chunk of filter f fills k_f entries per query of its
 * region.  So adl_bloom_probe_batch_k_workspace_bytes(n, F, k(bpk), stride) ==
 * adl_bloom_probe_batch_workspace_bytes(n, F, bpk, stride), every array where
 * the uniform plan has it, and a workspace sized for max_k serves every call
 * with a smaller max_k.  Eligibility, the read contract, the filter edge
 * cases (a 0-byte filter, one of 2^31 bits or more and an id >= num_filters
 * answer 0), stream order and ADL_ERR_WORKSPACE are adl_bloom_probe_batch_device's;
 * a batch that stays direct runs the direct kernel with d_filter_k, and the
 * two paths answer bit for bit the same.  A batch whose max_k is above
 * ADL_BLOOM_PROBE_BATCH_MAX_K (read again by adl_bloom_reload_knobs; 30: no
 * limit; not set: 2, the measured crossover at 2^24 queries, DESIGN.md §5 and
 * §8) stays direct as well, and its workspace size is 256; the size equation
 * above holds for every max_k the knob admits.
 *
 * max_k in 1..30; key_stride as for adl_bloom_probe_batch_workspace_bytes.
 * 256 for a batch that stays on the direct kernel; 0 for max_k outside 1..30. */
uint64_t adl_bloom_probe_batch_k_workspace_bytes(uint64_t n, uint32_t num_filters,
                                                 uint32_t max_k, uint32_t key_stride);

/* adl_bloom_probe_batch_device with a probe count per filter: d_filter_k[f] (device,
 * num_filters bytes, each in [1, max_k]; anything else is outside the contract, and the
 * binned path clamps it so that nothing outside the workspace is written). */
int adl_bloom_probe_batch_k_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                                   uint32_t key_stride, const uint32_t *d_filter_id, uint32_t num_filters,
                                   const uint8_t *d_bitmaps, const uint64_t *d_bitmap_off,
                                   const uint64_t *d_bitmap_end, const uint8_t *d_filter_k, uint32_t max_k,
                                   uint8_t *d_out, void *d_workspace, uint64_t workspace_bytes, void *stream);

/* Host-pointer convenience for adl_bloom_probe_device.  Synchronous. */
int adl_bloom_probe(const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t n,
                    uint32_t key_stride, int32_t bits_per_key, const uint8_t *h_bitmap,
                    uint64_t bitmap_bytes, uint8_t *h_out, void *stream);

/* ------------------------------------------------- device-resident filter sets */

/* A set of filters resident in device memory (the reader side: one set per
 * SSTable filter block, or many SSTables' filters for a multi-get).  Replaces
 * the mmapped, non-owning bitmaps FilterBlockReader probes
 * (src/filter_block.cpp:172-184, src/sstable.cpp:195-204). */
typedef struct adl_bloom_filter_set adl_bloom_filter_set;

/* Upload num_filters bitmaps: filter f = h_bitmaps[h_bitmap_off[f] ..
 * h_bitmap_off[f+1]) (HOST arrays, num_filters+1 offsets).  Synchronous. */
int adl_bloom_filter_set_create(const uint8_t *h_bitmaps, const uint64_t *h_bitmap_off,
                                uint32_t num_filters, int32_t bits_per_key,
                                adl_bloom_filter_set **out);

/* Probe n host keys; key i against filter h_filter_id[i], or against
 * `filter` for every key when h_filter_id is NULL.  h_out[i] = 0/1.
 * Synchronous on `stream`. */
int adl_bloom_filter_set_probe(const adl_bloom_filter_set *set, const uint8_t *h_keys,
                               const uint64_t *h_offsets, uint64_t n, uint32_t key_stride,
                               const uint32_t *h_filter_id, uint32_t filter, uint8_t *h_out,
                               void *stream);

/* Device views of a set, for callers that keep queries on the device and call
 * adl_bloom_probe_multi_device themselves. */
int adl_bloom_filter_set_device_view(const adl_bloom_filter_set *set, const uint8_t **d_bitmaps,
                                     const uint64_t **d_bitmap_off, uint32_t *num_filters);

int adl_bloom_filter_set_destroy(adl_bloom_filter_set *set);

/* ------------------------------------------- filter cache keyed by SSTable oid */

/* Device-resident filter blocks of many SSTables in one arena of
 * capacity_bytes, keyed by oid (any byte string, e.g. the SHA-256 file name),
 * least recently used evicted first, at most max_tables blocks: the filter
 * side of DB::table_cache_ (src/db.hpp:96-97, LRUCache src/cache.hpp:23-93).
 * Blocks of any bits_per_key share one cache: each is probed with the k of
 * its own "bf:" info, as FilterBlockReader::CreateFilterAlgorithm reads it per
 * block (src/filter_block.cpp:158-170), so a level of tables written under
 * different DBOptions::bits_per_key is served by one cache and one launch.
 * bits_per_key (>= 0) is kept for source compatibility and not otherwise
 * used.  Thread-safe (one mutex per cache). */
typedef struct adl_bloom_filter_cache adl_bloom_filter_cache;

int adl_bloom_filter_cache_create(uint64_t capacity_bytes, uint32_t max_tables, int32_t bits_per_key,
                                  adl_bloom_filter_cache **out);
int adl_bloom_filter_cache_destroy(adl_bloom_filter_cache *cache);

/* Insert (or replace) the filter block of table `oid`: validated as
 * FilterBlockReader::Init does (ADL_FILTER_BLOCK_ERROR); its bitmaps are
 * uploaded once, its k taken from its own bits_per_key, and it becomes the
 * most recently used.  Synchronous. */
int adl_bloom_filter_cache_put(adl_bloom_filter_cache *cache, const char *oid, uint64_t oid_len,
                               const uint8_t *h_block, uint64_t block_len);

/* 1 if cached (and now most recently used), else 0. */
int adl_bloom_filter_cache_contains(adl_bloom_filter_cache *cache, const char *oid, uint64_t oid_len);

/* 1 if removed, 0 if it was not cached. */
int adl_bloom_filter_cache_remove(adl_bloom_filter_cache *cache, const char *oid, uint64_t oid_len);

int adl_bloom_filter_cache_stats(adl_bloom_filter_cache *cache, uint32_t *tables, uint64_t *bytes_used);

/* Multi-get: query i (host keys) probes filter `filter` (0 for SSTables) of
 * table h_table[i], an index into the oid list oids[0..num_tables).  One
 * launch for the batch.  A query bound for a table that is not cached
 * answers 1 ("may be present": read the table); one bound for a filter the
 * block does not have answers 0 (src/filter_block.cpp:174).  *h_uncached
 * (optional) counts the queries whose table was not cached.  Synchronous.
 * Replaces SSTableReader::Get's filter check (src/sstable.cpp:238) across the
 * tables of a multi-get. */
int adl_bloom_filter_cache_probe(adl_bloom_filter_cache *cache, const char *const *oids,
                                 const uint64_t *oid_lens, uint32_t num_tables, uint32_t filter,
                                 const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t n,
                                 uint32_t key_stride, const uint32_t *h_table, uint8_t *h_out,
                                 uint64_t *h_uncached, void *stream);

/* The same multi-get with each key given once: key i (host keys, num_keys of
 * them) probes filter `filter` of every table of its candidate list,
 * h_pair_table[h_pair_begin[i] .. h_pair_begin[i+1]) (indices into the oid
 * list; h_pair_begin: num_keys+1 u32, h_pair_begin[0] == 0, non-decreasing --
 * anything else, or a table index >= num_tables, is ADL_ERR_INVALID_ARG).
 * h_out[p], one byte per pair in pair order, and *h_uncached (pairs bound for
 * tables that are not cached) are exactly what adl_bloom_filter_cache_probe
 * gives for the expanded (key, table) pairs; the keys cross the link and are
 * hashed once each instead of once per candidate table.  Batches of up to 8
 * pairs are expanded and served by adl_bloom_filter_cache_probe itself (the
 * resident server).  Synchronous.  Replaces Level::Get's loop over the
 * level's tables (src/revision.cpp:265-310) for a batch of lookup keys. */
int adl_bloom_filter_cache_probe_fanout(adl_bloom_filter_cache *cache, const char *const *oids,
                                        const uint64_t *oid_lens, uint32_t num_tables, uint32_t filter,
                                        const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t num_keys,
                                        uint32_t key_stride, const uint32_t *h_pair_begin,
                                        const uint32_t *h_pair_table, uint8_t *h_out, uint64_t *h_uncached,
                                        void *stream);

/* Bulk probe of DEVICE keys through the cache (a large existence check over
 * the cached tables): adl_bloom_probe_batch_k_device over the arena, each table
 * with the k of its own block, so a big batch takes the tile-binned pipeline.
 *
 * The workspace size for the largest k among the listed tables as they are
 * cached now (an uncached table: k 1); key_stride as for
 * adl_bloom_probe_batch_workspace_bytes. */
uint64_t adl_bloom_filter_cache_probe_batch_workspace_bytes(adl_bloom_filter_cache *cache,
        const char *const *oids, const uint64_t *oid_lens, uint32_t num_tables,
        uint64_t n, uint32_t key_stride);

/* Query i (DEVICE keys) probes filter `filter` of table d_table[i] (device u32, an index into the oid list).
 * Answers are adl_bloom_filter_cache_probe's for the same queries: 1 for a table that is not cached,
 * 0 for a filter the block does not have, 0 for an index >= num_tables, each table with the k of its own block.
 * h_cached (optional, num_tables bytes): 1 where the table was cached.  d_out: n bytes on the device.
 * The listed tables are resolved and pinned once, the range and k tables uploaded from the thread's staging,
 * the probe enqueued on `stream`, and the call returns after it has completed (the pins are held until then).
 * ADL_ERR_WORKSPACE: the workspace is smaller than this call's plan needs (a table was replaced by one of a
 * larger k since the size was asked): d_out is not written, the pins are given back; ask the size again. */
int adl_bloom_filter_cache_probe_batch_device(adl_bloom_filter_cache *cache, const char *const *oids,
        const uint64_t *oid_lens, uint32_t num_tables, uint32_t filter,
        const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n, uint32_t key_stride,
        const uint32_t *d_table, uint8_t *d_out, uint8_t *h_cached,
        void *d_workspace, uint64_t workspace_bytes, void *stream);

/* ------------------------------------------- resident level index */

/* A level described once -- where a revision installs it -- and asked about
 * many times: which of its tables Level::Get visits for a lookup key
 * (src/revision.cpp:278-287: files_meta_ ordered by min_inner_key, walked in
 * reverse, a table skipped when its [min_inner_key, max_inner_key] range does
 * not cover MemKey(user_key, seq, OP_PUT)).  The tables' boundary user keys
 * cut the key space into regions (a gap between two of them, or one of them);
 * the index holds the sorted boundaries and every region's candidate tables in
 * visiting order.  It does not depend on a lookup's seq: a table listed at its
 * own max user key carries its max (seq, op), and a lookup drops it when
 * max_seq > seq || (max_seq == seq && max_op > 0).  Immutable once created;
 * any number of threads may use one level at once.  The device copy is made
 * by the first device call on it (that one call waits for the upload on a
 * stream of the calling thread's; create and stats need no GPU). */
typedef struct adl_bloom_level adl_bloom_level;

/* Table t (an index < num_tables, the value the calls below report): its key
 * range as inner keys (user key + LE64 seq + op byte; a key shorter than 9
 * bytes is a user key with seq 0, op 0) and the oid its filter block is cached
 * under.  oids may be NULL (no adl_bloom_level_multiget then).  A table whose
 * max user key sorts before its min is never a candidate.  max_index_bytes:
 * the budget of the index, 0 = 256 MiB; heavily overlapping tables need
 * O(num_tables^2) list entries, and ADL_ERR_TOO_LARGE says the index would
 * exceed the budget (nothing is built: select on the host per batch instead),
 * or that a single key could have 2^24 candidates or more. */
int adl_bloom_level_create(const char *const *oids, const uint64_t *oid_lens, const char *const *min_inner_keys,
                           const uint64_t *min_lens, const char *const *max_inner_keys, const uint64_t *max_lens,
                           uint32_t num_tables, uint64_t max_index_bytes, adl_bloom_level **level);
/* No call on the level may be running or start once this is called. */
int adl_bloom_level_destroy(adl_bloom_level *level);

/* regions, entries of all region lists, the bytes of the device copy and the
 * longest list (each optional): no key has more candidates than
 * *longest_list, so num_keys * *longest_list pairs always suffice. */
int adl_bloom_level_stats(const adl_bloom_level *level, uint32_t *regions, uint64_t *list_entries,
                          uint64_t *device_bytes, uint32_t *longest_list);

/* Selection on the device: key i's candidate tables are d_pair_table
 * [d_pair_begin[i] .. d_pair_begin[i+1]) in visiting order.  Stream-ordered on
 * `stream` with no synchronisation (but see the first call, above):
 * d_pair_begin (num_keys+1
 * u32) and d_pair_table are the arrays adl_bloom_probe_fanout_device
 * consumes.  d_pair_begin is always complete and *d_num_pairs (a device u64)
 * the total needed; entries from pair_capacity on are not written.  A total
 * of 2^32 or more leaves d_pair_begin meaningless.  d_keys as for the probes:
 * any alignment, no byte outside a key is read.  d_workspace: 256-byte
 * aligned, adl_bloom_level_candidates_workspace_bytes(num_keys) bytes. */
uint64_t adl_bloom_level_candidates_workspace_bytes(uint64_t num_keys);
int adl_bloom_level_candidates_device(adl_bloom_level *level, const uint8_t *d_keys, const uint64_t *d_offsets,
                                      uint64_t num_keys, uint32_t key_stride, int64_t seq, uint32_t *d_pair_begin,
                                      uint32_t *d_pair_table, uint64_t pair_capacity, uint64_t *d_num_pairs,
                                      void *d_workspace, uint64_t workspace_bytes, void *stream);

/* Level multi-get: uploads the keys (and offsets) only; selection, list
 * expansion and the probes run on the device; h_pair_begin (num_keys+1),
 * h_pair_table and h_out (one byte per pair) come back.  The level's oids are
 * resolved and pinned in `cache` as adl_bloom_filter_cache_probe_fanout does
 * with its oid list, and the answers are that call's on the same lists: a
 * table that is not cached answers 1 and is counted in *h_uncached, a filter
 * the block does not have answers 0, each table is probed with the k of its
 * own block.  *num_pairs is the total; when it exceeds pair_capacity the call
 * returns ADL_ERR_WORKSPACE with h_pair_begin complete and nothing else
 * written, and ADL_ERR_TOO_LARGE when it is 2^32 or more.  Synchronous.
 * Replaces Level::Get's loop over the level's tables (src/revision.cpp:265-310)
 * and SSTableReader::Get's filter check for a batch of lookup keys. */
int adl_bloom_level_multiget(adl_bloom_level *level, adl_bloom_filter_cache *cache, uint32_t filter,
                             const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t num_keys,
                             uint32_t key_stride, int64_t seq, uint32_t *h_pair_begin, uint32_t *h_pair_table,
                             uint8_t *h_out, uint64_t pair_capacity, uint64_t *num_pairs, uint64_t *h_uncached,
                             void *stream);

/* ------------------------------------------- revision multi-get */

/* The whole revision asked once.  Revision::Get (src/revision.cpp:391-403)
 * walks its levels in order, level 0 first, skips a level that is Empty() and
 * calls Level::Get on the others until one finds the key.  A revision here is
 * the list of its levels' resident indices, in that visiting order; the levels
 * are BORROWED and must outlive it.  A NULL entry or a level of 0 tables is an
 * empty level.  Table t of level l has the GLOBAL id table_base[l] + t, where
 * table_base[l] counts the tables of the levels before l; every call below
 * reports global ids.  create, destroy and stats need no GPU; the device copy
 * (the non-empty levels' descriptors and bases) is made by the first device
 * call, which also makes each level's own copy. */
#define ADL_BLOOM_MAX_LEVELS 8
typedef struct adl_bloom_revision adl_bloom_revision;

/* ADL_ERR_INVALID_ARG: more than ADL_BLOOM_MAX_LEVELS levels.
 * ADL_ERR_TOO_LARGE: 2^31 - 1 tables or more in all, or the levels'
 * longest_list values sum to 2^24 or more (256 keys' lists add up in a u32,
 * as within one level). */
int adl_bloom_revision_create(adl_bloom_level *const *levels, uint32_t num_levels, adl_bloom_revision **rev);
/* No call on the revision may be running or start once this is called.  The
 * levels stay the caller's. */
int adl_bloom_revision_destroy(adl_bloom_revision *rev);
/* table_base: num_levels + 1 entries (the last: the tables of all levels).
 * *longest_list: the sum over the levels -- no key has more candidates, so
 * num_keys * *longest_list pairs always suffice.  Each optional. */
int adl_bloom_revision_stats(const adl_bloom_revision *rev, uint32_t *num_levels, uint32_t *table_base,
                             uint32_t *longest_list);

/* Selection over all levels on the device: key i's list is the concatenation,
 * level 0 first, of what adl_bloom_level_candidates_device gives for each
 * level at `seq`, as global ids.  The contract is that call's in every other
 * respect: d_pair_begin (num_keys+1 u32) always complete, entries from
 * pair_capacity on not written, *d_num_pairs the u64 total, no byte outside a
 * key read, stream-ordered with no synchronisation apart from the first call's
 * upload.  The number of launches does not depend on the number of levels.
 * Revision::Get takes a seq but does not pass it on (levels_[i].Get(key,
 * value), src/revision.cpp:395: Level::Get's default, INT64_MAX), so seq =
 * INT64_MAX reproduces the reference's Revision::Get itself.  d_workspace:
 * 256-byte aligned, adl_bloom_revision_candidates_workspace_bytes(rev,
 * num_keys) bytes. */
uint64_t adl_bloom_revision_candidates_workspace_bytes(const adl_bloom_revision *rev, uint64_t num_keys);
int adl_bloom_revision_candidates_device(adl_bloom_revision *rev, const uint8_t *d_keys, const uint64_t *d_offsets,
                                         uint64_t num_keys, uint32_t key_stride, int64_t seq,
                                         uint32_t *d_pair_begin, uint32_t *d_pair_table, uint64_t pair_capacity,
                                         uint64_t *d_num_pairs, void *d_workspace, uint64_t workspace_bytes,
                                         void *stream);

/* The fan-out probe that returns the survivors only: the inputs of
 * adl_bloom_probe_fanout_device; key i's hits are d_hit_filter[d_hit_begin[i]
 * .. d_hit_begin[i+1]), the d_pair_filter[p] of exactly those pairs p of key i
 * that adl_bloom_probe_fanout_device answers 1 for, in pair order.
 * d_hit_begin (num_keys+1 u32) is always complete and *d_num_hits (a device
 * u64) the total; entries from hit_capacity on are not written.  The output is
 * deterministic (a stable compaction: no atomic decides an order).
 * Stream-ordered, three launches; num_keys == 0 launches none.  d_workspace:
 * 256-byte aligned, adl_bloom_probe_fanout_hits_workspace_bytes(num_keys,
 * num_pairs) bytes (it holds the answer bytes). */
uint64_t adl_bloom_probe_fanout_hits_workspace_bytes(uint64_t num_keys, uint64_t num_pairs);
int adl_bloom_probe_fanout_hits_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t num_keys,
                                       uint32_t key_stride, const uint32_t *d_pair_begin,
                                       const uint32_t *d_pair_filter, uint64_t num_pairs, uint32_t num_filters,
                                       const uint8_t *d_bitmaps, const uint64_t *d_begin, const uint64_t *d_end,
                                       int32_t bits_per_key, uint32_t *d_hit_begin, uint32_t *d_hit_filter,
                                       uint64_t hit_capacity, uint64_t *d_num_hits, void *d_workspace,
                                       uint64_t workspace_bytes, void *stream);

/* Revision multi-get: uploads the keys (and offsets) only; selection over
 * every level, list expansion, the probes and the compaction of the hits run
 * on the device; h_hit_begin (num_keys+1) and h_hit_table come back: per key
 * the tables it still has to read, as global ids, the levels ascending and
 * within a level in Level::Get's order -- the order Revision::Get visits them
 * in.  The candidate pairs never leave the device: pair_capacity sizes their
 * scratch (0: min(num_keys * the revision's longest_list, 2^32-1)) and
 * *num_pairs reports their total; a total above pair_capacity is
 * ADL_ERR_WORKSPACE with *num_pairs set and nothing else written, one of 2^32
 * or more ADL_ERR_TOO_LARGE.  *num_hits above hit_capacity is
 * ADL_ERR_WORKSPACE with h_hit_begin complete.  The oids of all levels are
 * resolved and pinned in `cache` in one pass (a level created without oids:
 * ADL_ERR_INVALID_ARG); a table that is not cached answers 1, so it is a hit,
 * and *h_uncached counts such hits; a filter the block does not have answers
 * 0; each table is probed with the k of its own block, as
 * adl_bloom_level_multiget does.  num_keys == 0 launches nothing.
 * Synchronous.  Replaces Revision::Get's loop over the levels
 * (src/revision.cpp:391-403) up to the tables' filter checks for a batch of
 * lookup keys; reading the tables, and stopping at the first that holds the
 * key, stay with the caller, who walks the hits in order. */
int adl_bloom_revision_multiget(adl_bloom_revision *rev, adl_bloom_filter_cache *cache, uint32_t filter,
                                const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t num_keys,
                                uint32_t key_stride, int64_t seq, uint32_t *h_hit_begin, uint32_t *h_hit_table,
                                uint64_t hit_capacity, uint64_t *num_hits, uint64_t pair_capacity,
                                uint64_t *num_pairs, uint64_t *h_uncached, void *stream);

/* The hits of a multi-get grouped by table, on the device.  Level::Get reads
 * every candidate table of a level and keeps the smallest inner key
 * (src/revision.cpp:279-308), so each hit within a level is a certain read,
 * and each read opens its table's reader first (src/revision.cpp:289); a
 * batched reader therefore wants the hits table by table.  Input: the output
 * of adl_bloom_probe_fanout_hits_device -- d_hit_begin (num_keys+1 u32; H =
 * d_hit_begin[num_keys] is read on the device) and d_hit_table, ids <
 * num_tables, no id twice in one key's list.  Output: the G tables with at
 * least one hit in d_group_table, ascending by id (for a revision's global
 * ids: the levels ascending, src/revision.cpp:391-403); d_group_begin (G+1
 * entries); d_entry_key[d_group_begin[g] .. d_group_begin[g+1]) the indices
 * of the keys that hit d_group_table[g], ascending.  d_counts (two device
 * u64): [0] = H, [1] = G, always written.  Entries from entry_capacity on and
 * groups from group_capacity on (begins from group_capacity+1 on) are not
 * written; with H > entry_capacity nothing is grouped and only d_counts[0]
 * means anything.  Whatever the arrays hold (ids >= num_tables included),
 * nothing outside the outputs and the workspace is written.  The output is
 * deterministic (a stable radix sort on the id, 8 bits per pass, and a stable
 * compaction: no atomic decides a position).  Stream-ordered with no
 * synchronisation; four launches up to 256 tables, 4 + 3 *
 * ceil(bits(num_tables-1) / 8) beyond, whatever the arrays hold; num_keys == 0
 * launches none and reports 0 / 0.  ADL_ERR_TOO_LARGE: num_keys >= 2^32-1 or entry_capacity >=
 * 2^32.  d_workspace: 256-byte aligned (else ADL_ERR_INVALID_ARG),
 * adl_bloom_hits_by_table_workspace_bytes(num_keys, entry_capacity,
 * num_tables) bytes (fewer: ADL_ERR_WORKSPACE; the size is 0 for an
 * entry_capacity of 2^32 or more). */
uint64_t adl_bloom_hits_by_table_workspace_bytes(uint64_t num_keys, uint64_t entry_capacity, uint32_t num_tables);
int adl_bloom_hits_by_table_device(const uint32_t *d_hit_begin, const uint32_t *d_hit_table, uint64_t num_keys,
                                   uint32_t num_tables, uint32_t *d_group_table, uint32_t *d_group_begin,
                                   uint64_t group_capacity, uint32_t *d_entry_key, uint64_t entry_capacity,
                                   uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes, void *stream);

/* Revision multi-get that returns a read plan: adl_bloom_revision_multiget's
 * work (same arguments, same resolution and pinning of the oids, same answers)
 * followed by the grouping above, in one call.  h_group_table (*num_groups
 * global ids, ascending: the levels ascending), h_group_begin (*num_groups+1)
 * and h_entry_key (*num_hits key indices; group g's ascending) come back: the
 * tables to open, and for each the batch's keys to look up in it, in batch
 * order.  The reader walks the levels ascending (src/revision.cpp:391-403),
 * within a level visits each group once (every table of the level that
 * survives is read, src/revision.cpp:279-308) and skips the keys an earlier
 * level has found.  The key-major hit lists stay on the device beside the
 * candidate pairs, which pair_capacity sizes as for
 * adl_bloom_revision_multiget: a pair total above it is ADL_ERR_WORKSPACE with
 * *num_pairs set and nothing else written, one of 2^32 or more
 * ADL_ERR_TOO_LARGE.  *num_hits > entry_capacity or *num_groups >
 * group_capacity is ADL_ERR_WORKSPACE with both counts set (both exact) and
 * no array written.  A level created without oids: ADL_ERR_INVALID_ARG.
 * *h_uncached counts the entries whose table was not cached.  num_keys == 0
 * launches nothing (h_group_begin[0] = 0).  Synchronous. */
int adl_bloom_revision_read_plan(adl_bloom_revision *rev, adl_bloom_filter_cache *cache, uint32_t filter,
                                 const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t num_keys,
                                 uint32_t key_stride, int64_t seq, uint32_t *h_group_table, uint32_t *h_group_begin,
                                 uint64_t group_capacity, uint64_t *num_groups, uint32_t *h_entry_key,
                                 uint64_t entry_capacity, uint64_t *num_hits, uint64_t pair_capacity,
                                 uint64_t *num_pairs, uint64_t *h_uncached, void *stream);

/* ------------------------------------------- single-key revision Get */

/* DB::Get of one key is Revision::Get: every level's candidate tables asked
 * about the same key.  Up to ADL_BLOOM_GET_MAX_TABLES tables and a key of up
 * to ADL_BLOOM_GET_MAX_KEY_BYTES bytes travel in ONE request to the cache's
 * resident probe server (the key staged and hashed once, one lane per table,
 * one answer line, no launch); anything larger, and any request the server
 * does not take (switched off, missing, backing off, no answer in time), is
 * one launched fan-out probe with the same answers. */
#define ADL_BLOOM_GET_MAX_TABLES 24
#define ADL_BLOOM_GET_MAX_KEY_BYTES 96

/* One key against filter `filter` of every listed table: h_out[t] (num_tables
 * bytes) and *h_uncached are by definition those of
 * adl_bloom_filter_cache_probe_fanout for one key whose candidate list is
 * tables 0 .. num_tables-1 -- a table that is not cached answers 1 and is
 * counted, a filter the block does not have answers 0, each table is probed
 * with the k of its own block.  The tables are resolved and pinned for the
 * call as that call pins them.  num_tables == 0 does nothing.  h_key may be
 * NULL for key_len == 0.  Synchronous. */
int adl_bloom_filter_cache_probe_key(adl_bloom_filter_cache *cache, const char *const *oids,
                                     const uint64_t *oid_lens, uint32_t num_tables, uint32_t filter,
                                     const uint8_t *h_key, uint64_t key_len, uint8_t *h_out, uint64_t *h_uncached,
                                     void *stream);

/* GPU-free: the key's candidate tables over all levels, as global ids in
 * Revision::Get's visiting order -- what adl_bloom_revision_candidates_device
 * gives for this key at `seq` -- from the levels' host indices.  *num is the
 * total; entries from `capacity` on are not written (h_table may be NULL for
 * capacity == 0). */
int adl_bloom_revision_candidates_host(const adl_bloom_revision *rev, const uint8_t *h_key, uint64_t key_len,
                                       int64_t seq, uint32_t *h_table, uint32_t capacity, uint32_t *num);

/* adl_bloom_revision_multiget for one key: the tables the Get still has to
 * read, as global ids in visiting order, in h_hit_table; *num_hits above
 * hit_capacity is ADL_ERR_WORKSPACE with *num_hits (and *num_candidates) set
 * and nothing else written; a level created without oids or a NULL rev, cache,
 * num_hits (or h_key with key_len > 0, or h_hit_table with hit_capacity > 0)
 * is ADL_ERR_INVALID_ARG.  The candidates are selected on the host
 * (adl_bloom_revision_candidates_host), ONLY their oids are resolved and
 * pinned in `cache`, and they are probed by one
 * adl_bloom_filter_cache_probe_key-style request; no device copy of the
 * revision or its levels is made.  *num_candidates (optional): the candidate
 * tables; *h_uncached (optional): the hits whose table was not cached.
 * Nothing is allocated per call once the calling thread's scratch has grown.
 * Synchronous. */
int adl_bloom_revision_get(adl_bloom_revision *rev, adl_bloom_filter_cache *cache, uint32_t filter,
                           const uint8_t *h_key, uint64_t key_len, int64_t seq, uint32_t *h_hit_table,
                           uint32_t hit_capacity, uint32_t *num_hits, uint32_t *num_candidates, uint32_t *h_uncached,
                           void *stream);

/* ------------------------------------------- write-through builds into the cache */

/* A table's filter block built straight into a reserved range of the cache
 * arena (SSTableWriter::Final, src/sstable.cpp:58): the block comes back to
 * the host for the file, and the range is published under the table's oid
 * once that is known (the oid is the SHA-256 of the finished file).  No
 * re-upload of the block, and no window in which a freshly written table
 * answers "not cached".  A ticket stands for the built, unpublished range. */
typedef struct adl_bloom_cache_ticket adl_bloom_cache_ticket;

/* With ADL_BLOOM_SKIP_ADJACENT_DUPLICATES (1u) in one flags word: every build
 * key is probed again against the bitmap it went into
 * (adl_bloom_verify_device) before the block may go resident; a key that is
 * missing fails the build with ADL_FILTER_BLOCK_ERROR. */
#define ADL_BLOOM_CACHE_VERIFY 2u

/* Build num_filters filters from HOST keys (filter f = keys [key_begin[f],
 * key_begin[f+1]), HOST array of num_filters+1 entries) into a range of
 * round_up(max(block bytes, bitmap bytes + 1), 256) arena bytes, reserved as
 * adl_bloom_filter_cache_put reserves its range (least recently used blocks
 * are evicted for it), and write the block -- exactly
 * adl_bloom_filter_block_bytes bytes, byte-identical to
 * adl_bloom_filter_block_build_device followed by a D2H -- to h_block
 * (block_bytes smaller than that: ADL_ERR_INVALID_ARG).  Pinned key and block
 * buffers are DMAed directly, pageable ones staged through the thread's
 * pinned buffer.  A one-filter block is built in place (no staging, no pack
 * launch); the trailer is framed on the host.  *ticket receives the handle
 * for publish / abandon.  Unlike put, a build never waits for room that only
 * unpublished tickets hold (a thread holding two tickets would wait for
 * itself): it returns ADL_ERR_OUT_OF_MEMORY and leaves the cache as it was.
 * With ADL_BLOOM_CACHE_VERIFY the result is read before the call returns: on
 * a missing key the range is released, no ticket is made and the status is
 * ADL_FILTER_BLOCK_ERROR.  Unknown flag bits: ADL_ERR_INVALID_ARG.
 * Synchronous.
 *
 * A ticket nobody publishes or abandons holds its range like any block being
 * uploaded: a put in need of that room waits for it.  Destroying a cache
 * with tickets outstanding is the caller's error, as a running call is. */
int adl_bloom_filter_cache_build(adl_bloom_filter_cache *cache, const uint8_t *h_keys,
                                 const uint64_t *h_offsets, uint32_t key_stride, const uint64_t *key_begin,
                                 uint32_t num_filters, int32_t bits_per_key, uint32_t flags, uint8_t *h_block,
                                 uint64_t block_bytes, adl_bloom_cache_ticket **ticket, void *stream);

/* Device bytes adl_bloom_filter_cache_build_device needs (>=
 * adl_bloom_filter_block_workspace_bytes); 0 on invalid input or a block
 * beyond the reference's int offsets. */
uint64_t adl_bloom_filter_cache_build_workspace_bytes(const uint64_t *key_begin, uint32_t num_filters,
                                                      int32_t bits_per_key);

/* The same build from DEVICE keys: enqueues on `stream` and does not
 * synchronise.  h_block may be NULL (no download); otherwise the bitmaps are
 * copied into it on `stream` (pinned memory keeps that asynchronous) and the
 * trailer is written by the host before the call returns, so the block is
 * complete once the stream's work is.  d_workspace (256-byte aligned) must
 * stay untouched until then.  adl_bloom_filter_cache_publish waits for the
 * build itself (an event recorded on `stream`), and with
 * ADL_BLOOM_CACHE_VERIFY reads the verify result there. */
int adl_bloom_filter_cache_build_device(adl_bloom_filter_cache *cache, const uint8_t *d_keys,
                                        const uint64_t *d_offsets, uint32_t key_stride,
                                        const uint64_t *key_begin, uint32_t num_filters, int32_t bits_per_key,
                                        uint32_t flags, void *d_workspace, uint64_t workspace_bytes,
                                        uint8_t *h_block, uint64_t block_bytes, adl_bloom_cache_ticket **ticket,
                                        void *stream);

/* adl_bloom_filter_cache_build with a stream (adl_bloom_stream, above) as its
 * key source: the filters of adl_bloom_stream_counts are built from the
 * stream's hash pairs straight into the reserved range -- nothing is uploaded
 * or hashed -- and the block, the bytes adl_bloom_filter_cache_build writes
 * for the same keys and bounds, goes to h_block.  *block_bytes receives its
 * length (block_capacity smaller: ADL_ERR_INVALID_ARG, with *block_bytes
 * set).  Flags, statuses and the ticket's publish / abandon life cycle are
 * adl_bloom_filter_cache_build's; ADL_BLOOM_CACHE_VERIFY probes every pair
 * again.  Runs behind every earlier append of the stream; the stream is not
 * consumed.  Synchronous (stream == NULL: the calling thread's own stream). */
int adl_bloom_filter_cache_build_stream(adl_bloom_filter_cache *cache, adl_bloom_stream *s, int32_t bits_per_key,
                                        uint32_t flags, uint8_t *h_block, uint64_t block_capacity,
                                        uint64_t *block_bytes, adl_bloom_cache_ticket **ticket, void *stream);

/* Make the built block the most recently used block of table `oid`,
 * replacing one cached under that oid; max_tables is enforced as in put.
 * Waits for the build's work first.  A device-variant build made with
 * ADL_BLOOM_CACHE_VERIFY that has a missing key releases the range instead
 * and returns ADL_FILTER_BLOCK_ERROR.  The ticket is consumed whatever the
 * status (except ADL_ERR_INVALID_ARG for a NULL argument). */
int adl_bloom_filter_cache_publish(adl_bloom_filter_cache *cache, adl_bloom_cache_ticket *ticket,
                                   const char *oid, uint64_t oid_len);

/* Give the range back (waits for the build's work first).  Consumes the ticket. */
int adl_bloom_filter_cache_abandon(adl_bloom_filter_cache *cache, adl_bloom_cache_ticket *ticket);

/* Construction check: probe every build key against the filter it belongs
 * to.  Key i (of n) belongs to filter f with d_key_begin[f] <= i <
 * d_key_begin[f+1] (DEVICE array, num_filters+1 entries, non-decreasing);
 * filter f = d_bitmaps[d_begin[f] .. d_end[f]) as in
 * adl_bloom_probe_ranges_device (d_end == NULL: d_begin has num_filters+1
 * entries).  d_result[0] = the number of keys the probe answers 0 for,
 * d_result[1] = the index of the first of them, or ~0 when there is none: 0
 * and ~0 after any correct build.  A key whose filter is empty or has 2^31
 * bits or more counts as missing (the probe would answer 0); a key outside
 * [d_key_begin[0], d_key_begin[num_filters]) was not built into any filter
 * and is not checked.  d_result is initialised on `stream` before the launch. */
int adl_bloom_verify_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n, uint32_t key_stride,
                            const uint64_t *d_key_begin, uint32_t num_filters, const uint8_t *d_bitmaps,
                            const uint64_t *d_begin, const uint64_t *d_end, int32_t bits_per_key,
                            uint64_t *d_result, void *stream);

/* Host-pointer convenience: filter f = h_bitmaps[h_bitmap_off[f] ..
 * h_bitmap_off[f+1]) (HOST arrays; key_begin and h_bitmap_off have
 * num_filters+1 entries).  *first_missing = ~0 when *missing = 0.  Synchronous. */
int adl_bloom_verify(const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t n, uint32_t key_stride,
                     const uint64_t *key_begin, uint32_t num_filters, const uint8_t *h_bitmaps,
                     const uint64_t *h_bitmap_off, int32_t bits_per_key, uint64_t *missing,
                     uint64_t *first_missing, void *stream);

/* ---------------------------------------------------------------- hash */

/* The reference's murmur3 variant (src/murmur3_hash.cpp:11-65) on the GPU for a
 * batch: d_out[2i] = murmur3_hash(seed_a, key_i), d_out[2i+1] = (seed_b, key_i). */
int adl_bloom_murmur3_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                             uint32_t key_stride, uint32_t seed_a, uint32_t seed_b,
                             uint32_t *d_out, void *stream);

/* Single-key form of murmur3_hash(seed, data, len) (src/murmur3_hash.hpp:9),
 * computed on the GPU.  Synchronous; on failure *h_out is left untouched. */
int adl_bloom_murmur3(uint32_t seed, const void *data, uint64_t len, uint32_t *h_out);

/* The calling thread's current HIP device (every device pointer above belongs
 * to it), and setting it: for host code that hands a build to another thread
 * (SSTableWriter::BeginFinal's worker), whose current device starts at 0. */
int adl_bloom_get_device(int32_t *device);
int adl_bloom_set_device(int32_t device);

/* ---------------------------------------------------------------- instrumentation */

/* Per-kernel timing of the build for the calling thread: while enabled, each
 * build takes start/stop timestamps of pass A (bloom_bin_kernel) and pass B
 * (bloom_tile_kernel) from their dispatch packets (hipExtLaunchKernel events,
 * nothing extra enqueued between the launches); up to `capacity` builds are kept.  collect()
 * synchronises on the recorded events, writes the summed milliseconds of the
 * two kernels to ms[0] (pass A) and ms[1] (pass B), the number of timed builds
 * to *builds, and disables timing.  Used by bench.py for the live roofline. */
int adl_bloom_profile_enable(uint32_t capacity);
int adl_bloom_profile_collect(double *ms, uint32_t *builds);
/* The same timings one launch pair at a time, without stopping: ms_ab[2i] =
 * pass A and ms_ab[2i+1] = pass B of pair i, for up to `capacity` pairs (for
 * medians); call before adl_bloom_profile_collect. */
int adl_bloom_profile_each(double *ms_ab, uint32_t capacity, uint32_t *launch_pairs);

/* Bit-sets a build wrote as positions (pass A's output, after it skipped
 * repeated hash pairs), read back from d_workspace, the workspace of a
 * *_device build made with these key counts and bits_per_key: *positions =
 * the sum over its chunks.  The build leaves the layout of its tables in the
 * workspace itself, so the answer is that workspace's last build's whatever
 * else the calling thread has built since, on this or another stream; a
 * workspace no build has run in is ADL_ERR_INVALID_ARG.  `stream` means what
 * it means to the *_device build (NULL = the null stream): pass the build's
 * stream and the readback is ordered after the build with no synchronise in
 * between.  Synchronous on `stream`.  For the bench's traffic accounting
 * (profiles/).
 * (Changed without a new ADL_BLOOM_ABI_VERSION, the signature and every
 * structure being what they were: NULL used to mean the calling thread's own
 * non-blocking stream here, which did not wait for a build on the null stream,
 * and the layout used to be that of the calling thread's last build, so a
 * workspace without a build was read as whatever that was instead of being
 * refused.) */
int adl_bloom_build_positions(const uint64_t *key_counts, uint32_t num_filters, int32_t bits_per_key,
                              const void *d_workspace, uint64_t *positions, void *stream);

/* Test-only fault injection (the error-path tests; never set by the product).
 * ADL_TEST_FAULT_PIPELINE_GROUP, arg g >= 0: the next adl_bloom_build_segmented
 * call fails in its group g's build, with earlier groups' copies in flight.
 * ADL_TEST_FAULT_CACHE_COMPLETION, arg >= 0: the next filter-cache probe that
 * waits for its answers in the mapped buffer sees its kernel's completion
 * report a device error after all answers have arrived.
 * ADL_TEST_FAULT_CACHE_BUILD_CORRUPT, arg >= 0: the next write-through cache
 * build clears the first non-zero byte of filter 0's bitmap in its arena
 * range, after the build and before verification (corrupted data, nothing
 * faults): the only way to see ADL_BLOOM_CACHE_VERIFY reject a build.
 * ADL_TEST_FAULT_SERVER_SEQ, arg v >= 0: no failure, a counter preset.  The
 * calling thread's next request to a resident probe server (any cache's)
 * continues its slot's sequence from v & 0x3FFFFFFF, as if that slot had
 * served so many requests: the request carries v + 1, so the tests reach the
 * answer tag's wrap at 2^24 and the sequence number's at 2^30 (which skips 0)
 * without the minutes of Gets either takes.  Kept per thread (a slot belongs
 * to the thread that posts into it) and taken once, by that thread's next
 * served-path request only.  It stores the counter and nothing else.
 * arg < 0 disarms.
 * (ADL_TEST_FAULT_SERVER_SEQ was added without a new ADL_BLOOM_ABI_VERSION:
 * the signature is unchanged and the value was rejected before.) */
#define ADL_TEST_FAULT_PIPELINE_GROUP 1
#define ADL_TEST_FAULT_CACHE_COMPLETION 2
#define ADL_TEST_FAULT_CACHE_BUILD_CORRUPT 3
#define ADL_TEST_FAULT_SERVER_SEQ 4
int adl_bloom_test_fault(int site, int64_t arg);

/* The tuning and test switches (ADL_BLOOM_* environment variables, DESIGN.md
 * §8) are read once per process, at the first call that needs them.  This
 * reads them again (tests that change them; no other call of the library may
 * be running). */
int adl_bloom_reload_knobs(void);

/* Resident probe server kernels launched by this process so far (first
 * launches and relaunches after an idle or life-limit exit), for the latency
 * tests (readpath_test --tails). */
int adl_bloom_probe_server_launches(uint64_t *launches);

/* (instrumentation) The resident probe server's request phases, averaged over
 * the requests since the last reset: *requests served, *stamped of them with
 * the kernel's stamps read back, and avg_us[7] = the kernel's gap since its
 * previous poll, then from the poll that found the request: its loads back,
 * the slot staged in LDS, the hashes done, the bit reads back, the answer
 * stored; avg_us[6] = the host's time per request (the request written to the
 * answer read).  reset != 0 clears the counters after reading them. */
int adl_bloom_probe_server_phases(uint64_t *requests, uint64_t *stamped, double *avg_us, int reset);

/* ---------------------------------------------------------------- synthetic data */

/* SURVEY.md §8d SplitMix64 16-byte keys, generated on the device: key i of the
 * stream seeded `seed`, skipping the first `skip` keys, = LE64(next) || LE64(next). */
int adl_synth_keys16_device(uint8_t *d_out, uint64_t seed, uint64_t skip, uint64_t n,
                            void *stream);

/* Variable-length synthetic keys (DESIGN.md "Synthetic inputs"): lengths
 * 8 + (r-1), r ~ Zipf(s) on [1, 249] by inverse CDF over a SplitMix64 counter
 * stream; d_lengths (n entries, uint32) must then be prefix-summed by the
 * caller into offsets, after which adl_synth_varlen_fill_device writes the
 * bytes (byte j of the packed buffer = byte j%8 of SplitMix64 output j/8). */
int adl_synth_varlen_lengths_device(uint32_t *d_lengths, uint64_t seed, uint64_t n, double zipf_s,
                                    void *stream);
int adl_synth_varlen_fill_device(uint8_t *d_out, uint64_t seed, uint64_t total_bytes, void *stream);

/* Probe queries of BASELINE.json configs[4] (DESIGN.md "Synthetic inputs"):
 * global query q = q0 + i draws four SplitMix64 outputs of the stream seeded
 * `seed` (calls 4q+1 .. 4q+4): r0 -> filter id r0 % num_tables; r1 odd -> an
 * inserted key, key j = (r1 >> 1) % keys_per_table of table t's key stream
 * (adl_synth_keys16_device(seed = table_seed0 + t)); r1 even -> a fresh key
 * LE64(r2) || LE64(r3).  d_member[i] = 1 for inserted keys (may be NULL). */
int adl_synth_probe_queries_device(uint8_t *d_keys, uint32_t *d_filter_id, uint8_t *d_member,
                                   uint64_t seed, uint64_t q0, uint64_t n, uint32_t num_tables,
                                   uint64_t table_seed0, uint64_t keys_per_table, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ADL_BLOOM_H_ */
