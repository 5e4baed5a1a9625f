/*
 * adacodec.h — C ABI of libadacodec: the MI355X (gfx950) succinct column-segment codec.
 *
 * This is the drop-in boundary for ONE path of leonwind/duckdb-adaptive-compression: the per-segment
 * bit-packed integer codec behind DuckDB's COMPRESSION_SUCCINCT function table.  Every entry point names
 * the reference interface it replaces (paths relative to the reference checkout).  Plain C types only:
 * pointers named d_* are DEVICE pointers (HBM), everything else is host memory.  No entry point falls back
 * to a CPU implementation: without a usable gfx950 device the device functions return ADAC_ERR_NO_DEVICE.
 *
 * Packed format (identical to sdsl::int_vector<0>, third_party/sdsl/include/sdsl/int_vector.hpp:289-327,
 * bits.hpp:456-529): value i of a segment occupies bits [i*w, (i+1)*w) of a little-endian uint64 stream,
 * LSB first, may straddle one word boundary; stored value = (x - min) mod 2^w; bits past count*w in the last
 * word are zero.  The integration glue (C++ adapter a DuckDB maintainer would add) is in INTEGRATION.md.
 */
#ifndef ADACODEC_H
#define ADACODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADAC_ABI_VERSION 1

typedef enum adac_status {
	ADAC_OK = 0,
	ADAC_ERR_INVALID_ARGUMENT = 1,
	ADAC_ERR_UNSUPPORTED_TYPE = 2, /* InternalException("Unsupported type ...") succinct.cpp:364 */
	ADAC_ERR_DEVICE = 3,           /* a HIP call failed; adac_last_error() has the text */
	ADAC_ERR_OUT_OF_MEMORY = 4,
	ADAC_ERR_NO_DEVICE = 5
} adac_status;

/* duckdb::PhysicalType codes of the eight supported types (src/include/duckdb/common/types.hpp:117-138;
 * supported set: SuccinctFun::TypeIsSupported, src/storage/compression/succinct.cpp:368-382). */
typedef enum adac_type {
	ADAC_UINT8 = 2,
	ADAC_INT8 = 3,
	ADAC_UINT16 = 4,
	ADAC_INT16 = 5,
	ADAC_UINT32 = 6,
	ADAC_INT32 = 7,
	ADAC_UINT64 = 8,
	ADAC_INT64 = 9
} adac_type;

/* Which of the reference's two encode paths produced / should produce a segment's min, max and width. */
typedef enum adac_rule {
	/* SuccinctAppendLoop + BitCompressFromSuccinct (succinct.cpp:271-306, column_segment.cpp:348-383):
	 * min/max over uint64_t(T x) (sign-extended for signed T), NULL rows excluded; w = hi(max-min)+1. */
	ADAC_RULE_APPEND = 0,
	/* BitCompressFromUncompressed (column_segment.cpp:385-456): min/max over the raw block zero-extended,
	 * NULL slots (NullValue<T>) included; max reduced by min only when max > min, so a constant non-zero
	 * segment keeps w = hi(value)+1. */
	ADAC_RULE_RECOMPACT = 1,
	/* Not an encode rule: typed min/max of the valid rows in T's own order — the segment zonemap
	 * (NumericStatistics::Update<T>, src/include/duckdb/storage/statistics/numeric_statistics.hpp:54-67, read by
	 * RowGroup::CheckZonemapSegments, src/storage/table/row_group.cpp:287-322).  adac_zonemap only. */
	ADAC_RULE_ZONEMAP = 2
} adac_rule;

#define ADAC_NO_MIN UINT64_MAX /* ColumnSegment::min_factor initial value: no frame of reference */
#define ADAC_SEG_PACKED 0x1u   /* width < 8*sizeof(T) and (x - min) stored; clear = raw slots at 8*sizeof(T) */

/* One column segment as the device sees it (32 bytes).  Mirrors the succinct members of
 * duckdb::ColumnSegment (src/include/duckdb/storage/table/column_segment.hpp:60-64,190-214):
 * succinct_vec.{data,width}, count, min_factor, compacted. */
typedef struct adac_segment_desc {
	uint64_t word_off; /* first uint64 word of the segment in the packed arena; multiple of 16 (128 B) */
	uint64_t val_off;  /* first element of the segment in the raw / decoded value buffer */
	uint64_t min;      /* min_factor, ADAC_NO_MIN if none */
	uint32_t count;    /* values in the segment */
	uint8_t width;     /* bits per stored value, 1..64 */
	uint8_t flags;     /* ADAC_SEG_* */
	uint16_t reserved;
} adac_segment_desc;

typedef struct adac_ctx adac_ctx;       /* one device + one HIP stream */
typedef struct adac_layout adac_layout; /* a batch of segments: counts, placement, device tables */

/* ---------------------------------------------------------------------------------------------
 * Host-only helpers (never touch the device).
 * ------------------------------------------------------------------------------------------- */

int adac_abi_version(void);
const char *adac_status_string(adac_status s);
const char *adac_last_error(void); /* thread-local text of the last ADAC_ERR_DEVICE */

/* SuccinctFun::TypeIsSupported (succinct.cpp:368-382) */
int adac_type_is_supported(int physical_type);
/* GetTypeIdSize for the supported types; 0 if unsupported */
uint32_t adac_type_size(int physical_type);
/* sdsl::bits::hi (bits.hpp:392-397): index of the highest set bit, hi(0) == 0 */
uint32_t adac_hi(uint64_t x);
/* Minimal width for a segment: column_segment.cpp:351-359 (rule APPEND) / :404-417 (rule RECOMPACT);
 * pad_to_byte = DBConfig::succinct_padded_to_next_byte_enabled (config.hpp:193). */
uint8_t adac_width(uint64_t min, uint64_t max, int rule, int pad_to_byte);
/* The min a PACKED descriptor stores for a segment analysed to (min, max) and planned at `width`: min itself,
 * except for the sentinel collision min == max == UINT64_MAX (every valid row is all-ones, -1 for the INT types):
 * the reference packs such a segment without subtracting and scans it without adding (UINT64_MAX doubles as "no
 * min": column_segment.cpp:371-373, succinct.cpp:138-140), returning 2^width - 1 instead of -1.  The product
 * keeps those packed bits and stores min = UINT64_MAX - (2^width - 1), which decodes them to the original value.
 * adac_plan applies this on the device; hosts that build descriptors themselves (adac_layout_set_descs) call it. */
uint64_t adac_stored_min(uint64_t min, uint64_t max, uint8_t width);

/* ceil(count*width/64): logical uint64 words of a packed segment (int_vector::capacity()/64) */
uint64_t adac_packed_words(uint64_t count, uint8_t width);
/* sdsl::size_in_bytes(succinct_vec) = 9 + 8*ceil(count*width/64) (io.hpp:636-640,
 * int_vector.hpp:602-609,1565-1578): what ColumnSegment::GetDataSize reports (column_segment.cpp:204-214) */
uint64_t adac_size_in_bytes(uint64_t count, uint8_t width);
/* words a segment occupies in the packed arena: the SDSL allocation ((bits+64)>>6 words,
 * memory_management.hpp:353) rounded up to 128 B */
uint64_t adac_arena_words(uint64_t count, uint8_t width);
/* Persistent block image of one packed segment (the reference never defined one: ConvertToPersistent is a
 * no-op for SUCCINCT, src/storage/table/column_segment.cpp:531-533).  Layout, little-endian:
 *   [0, 9 + 8*W)   the sdsl::int_vector<0> serialisation of the packed vector — uint64 bit_size, uint8 width,
 *                  W = ceil(bit_size/64) words (int_vector.hpp:602-609,1546-1578): sdsl::load() reads it back
 *   then 16 bytes  uint64 min_factor, uint8 flags (ADAC_SEG_*), uint8 physical type, 6 zero bytes
 * adac_size_in_bytes(count, width) + 16 bytes in total.  Host memory only. */
#define ADAC_BLOCK_TRAILER_BYTES 16
uint64_t adac_block_bytes(uint64_t count, uint8_t width);
/* words: the segment's ceil(count*width/64) packed words (host copy).  Returns bytes written, 0 if cap is short. */
uint64_t adac_block_write(const adac_segment_desc *desc, int physical_type, const uint64_t *words, void *out,
                          uint64_t cap);
/* Parses a block: fills desc (count, width, min, flags; word_off/val_off left 0), *physical_type, and copies
 * the packed words to words_out (capacity cap_words).  ADAC_ERR_INVALID_ARGUMENT on a malformed block. */
adac_status adac_block_read(const void *block, uint64_t len, adac_segment_desc *desc, int *physical_type,
                            uint64_t *words_out, uint64_t cap_words);

/* Header + trailer of a block image without touching its words (len: adac_block_bytes or adac_block_stride of
 * the image): what a loader needs to size the arena before adac_blocks_read moves the words. */
adac_status adac_block_peek(const void *block, uint64_t len, adac_segment_desc *desc, int *physical_type);
/* Bytes an image occupies in a block buffer: adac_block_bytes rounded up to whole 8-byte units (zero padded),
 * 8 * (packed_words + 4).  Images are placed at byte offsets that are multiples of 8. */
uint64_t adac_block_stride(uint64_t count, uint8_t width);

/* values per device tile for a type (16 KiB of decoded output) */
uint32_t adac_tile_values(int physical_type);
/* Launch-shape knobs for in-process A/B measurement: "templated_scan" (0/1), "scan_tiles_per_wg" (tiles per fused-scan
 * workgroup; 0 = chosen by type), "num_cus" (0 = the device's own count), "single_pass_encode" (0 = analyze + plan +
 * pack as three kernels), "encode_big_image", "encode_publish_ahead", "scan_cells", "tile_records", "gather_compact",
 * "group_sum_wide", "group_sum_rw", "group_product_rw", "group_product3_rw", "group_q1_rw", "group_dense_combine",
 * "group_dense_window", "group_mapped_copies" (copies of the mapped scans' on-chip bins; 0 = as many as fit),
 * "sel_debug": the table in
 * adac_set_tuning is the full list, Tuning in
 * csrc/adac_internal.h says what each does.  Decoded values, packed words, widths and mins never depend on them.  One
 * knob changes WHERE adac_encode puts a segment in the arena: "encode_placement" 1 hands out arena space in order of
 * completion (a cursor, no ordered look-back) instead of the exclusive prefix in segment order that adac_plan computes:
 * descriptors then carry offsets that differ from run to run (disjoint, 128-byte aligned, inside max_arena_words).
 * "encode_stamps" 1 records diagnostic time stamps.  Returns 0 if the name is known and the value accepted
 * ("scan_tiles_per_wg" and "num_cus" refuse negative values), 1 otherwise. */
int adac_set_tuning(const char *name, int value);
/* Diagnostic, not part of the drop-in boundary: the phase time stamps (8 x uint64 per segment) the single-pass encode
 * recorded while "encode_stamps" was set (tools/encode_stamps.py).  Returns 0 on success. */
int adac_debug_encode_stamps(void *host, uint64_t bytes);

/* ---------------------------------------------------------------------------------------------
 * Context and device memory.
 *
 * Threading: a context is one HIP stream and a layout caches launch tables on it, so calls that share a context
 * (or a layout) are serialised by the caller — the host mirror does it with its pool lock, the way the
 * reference serialises representation flips with bit_compression_lock (column_segment.cpp:162-167).  Different
 * contexts (one per engine worker, or one per GPU) are independent; the host-only helpers are re-entrant.
 * ------------------------------------------------------------------------------------------- */

/* gfx950 devices visible to this process (hipGetDeviceCount); 0 when there is none or the runtime is unusable.
 * A host builds one segment pool per device from it. */
int adac_device_count(void);

/* Binds to HIP device `device`.  external_stream: a hipStream_t owned by the caller (e.g. the engine's or
 * torch's current stream) or NULL to create a private non-blocking stream. */
adac_status adac_ctx_create(int device, void *external_stream, adac_ctx **out);
/* Layouts, plans and graphs hold a reference on their context: adac_ctx_destroy drops the creator's reference and
 * the stream goes away with the last object made on it, so destruction order does not matter.  Raw device memory
 * (adac_dev_alloc) is not tracked: free it before the context. */
void adac_ctx_destroy(adac_ctx *ctx);
adac_status adac_ctx_sync(adac_ctx *ctx);
void *adac_ctx_stream(adac_ctx *ctx); /* the hipStream_t every launch of this ctx goes to */
int adac_ctx_device(adac_ctx *ctx);

adac_status adac_dev_alloc(adac_ctx *ctx, size_t bytes, void **d_ptr);
adac_status adac_dev_free(adac_ctx *ctx, void *d_ptr);
adac_status adac_dev_memset(adac_ctx *ctx, void *d_ptr, int byte, size_t bytes);   /* stream-ordered */
adac_status adac_memcpy_h2d(adac_ctx *ctx, void *d_dst, const void *src, size_t bytes); /* blocking */
adac_status adac_memcpy_d2h(adac_ctx *ctx, void *dst, const void *d_src, size_t bytes); /* blocking */

/* Device-to-host copy enqueued on the context's stream without waiting for it (dst should be page-locked,
 * adac_host_alloc_pinned, for the copy to overlap host work); adac_ctx_sync makes the bytes visible. */
adac_status adac_memcpy_d2h_async(adac_ctx *ctx, void *dst, const void *d_src, size_t bytes);
/* Page-locked host memory for staging (hipHostMalloc): D2H/H2D copies of it run at PCIe line rate. */
adac_status adac_host_alloc_pinned(adac_ctx *ctx, size_t bytes, void **ptr);
adac_status adac_host_free_pinned(adac_ctx *ctx, void *ptr);

/* A marker in a context's stream: adac_event_record enqueues it, adac_event_wait blocks the calling host thread until
 * everything enqueued before it has finished (and only that: later work on the same stream is not waited for, which
 * is what lets a host keep several decode + copy batches in flight on one stream).  Any thread may wait. */
typedef struct adac_event adac_event;
adac_status adac_event_record(adac_ctx *ctx, adac_event **out);
adac_status adac_event_wait(adac_event *ev);
int adac_event_done(adac_event *ev); /* 1 finished, 0 still running (or error) */
void adac_event_destroy(adac_event *ev);

/* HIP-event stopwatch on the ctx stream (for measuring kernels where they are launched). */
adac_status adac_timer_start(adac_ctx *ctx);
adac_status adac_timer_stop(adac_ctx *ctx, float *elapsed_ms); /* records, synchronises, reads */

/* ---------------------------------------------------------------------------------------------
 * Layout: a batch of segments of one physical type.
 * ------------------------------------------------------------------------------------------- */

/* counts[i]: values in segment i (ColumnSegment::count).  val_offs[i]: element offset of segment i in the
 * value buffer handed to analyze/pack/unpack, or NULL for back-to-back placement.  Builds the device tile
 * table; descriptors start with width = 8*sizeof(T), min = ADAC_NO_MIN, not packed (the state of a fresh
 * transient SUCCINCT segment, column_segment.cpp:101-105). */
adac_status adac_layout_create(adac_ctx *ctx, int physical_type, const uint32_t *counts, const uint64_t *val_offs,
                               uint64_t nseg, adac_layout **out);
void adac_layout_destroy(adac_layout *l);
uint64_t adac_layout_nseg(const adac_layout *l);
uint64_t adac_layout_ntiles(const adac_layout *l);
uint64_t adac_layout_total_values(const adac_layout *l);
/* elements the value buffer must hold: max(val_off + count) */
uint64_t adac_layout_value_span(const adac_layout *l);
/* upper bound of the packed arena in uint64 words for ANY widths (every segment unpacked) */
uint64_t adac_layout_max_arena_words(const adac_layout *l);
/* Upload host descriptors (decode of segments encoded elsewhere). word_off must be a multiple of 16. */
adac_status adac_layout_set_descs(adac_layout *l, const adac_segment_desc *descs);
/* Download the device descriptors (after adac_plan / adac_encode).  Synchronises the stream. */
adac_status adac_layout_get_descs(adac_layout *l, adac_segment_desc *descs);
/* Download per-segment {min,max} pairs (2*nseg uint64) left by adac_analyze.  Synchronises. */
adac_status adac_layout_get_minmax(adac_layout *l, uint64_t *minmax);
/* The device copy of the descriptor table (nseg entries), for callers that chain their own kernels. */
const adac_segment_desc *adac_layout_device_descs(const adac_layout *l);

/* ---------------------------------------------------------------------------------------------
 * Hot path.  All calls enqueue on the ctx stream and return without synchronising.
 * ------------------------------------------------------------------------------------------- */

/* Per-segment min/max.  Replaces the running min/max of SuccinctAppendLoop (succinct.cpp:271-306; rule
 * APPEND) and pass 1 of BitCompressFromUncompressed (column_segment.cpp:390-400; rule RECOMPACT).
 * d_vals: raw values of type T at element offsets val_off.  d_validity: DuckDB validity mask over the same
 * element index space (bit e of word e/64 set = row valid) or NULL = all valid. */
adac_status adac_analyze(adac_layout *l, const void *d_vals, const uint64_t *d_validity, int rule);

/* Segment zonemaps: zonemap[2*s] / [2*s+1] = minimum / maximum of segment s over its valid rows, as bit patterns
 * of T (zero-extended), ordered as T orders them (signed for the INT types).  A segment without a valid row
 * reports min = T's maximum and max = T's minimum (an empty interval).  Overwrites the layout's min/max
 * scratch (run it before or after an encode, not between adac_analyze and adac_plan).  Synchronises. */
adac_status adac_zonemap(adac_layout *l, const void *d_vals, const uint64_t *d_validity, uint64_t *zonemap);

/* From the min/max left by adac_analyze compute every segment's width, flags, stored min and arena offset
 * on the device (no host round trip).  Replaces the width decision of column_segment.cpp:351-363 /
 * :404-420.  A segment whose width would not shrink (8*sizeof(T) <= w) stays unpacked. */
adac_status adac_plan(adac_layout *l, int rule, int pad_to_byte);

/* Bit-pack every segment: words[word_off + ...] <- (x - min) mod 2^w.  Replaces the pack loops of
 * BitCompressFromSuccinct (column_segment.cpp:365-376) and BitCompressFromUncompressed (:426-443).
 * NULL slots are stored as NullValue<T> - min (succinct.cpp:288-291, null_value.hpp:26-28). */
adac_status adac_pack(adac_layout *l, const void *d_vals, const uint64_t *d_validity, uint64_t *d_words);

/* analyze + plan + pack */
adac_status adac_encode(adac_layout *l, const void *d_vals, const uint64_t *d_validity, int rule, int pad_to_byte,
                        uint64_t *d_words);

/* Re-compaction packed -> packed (the `adac_repack(words, n, old_w, new_w, min)` of SURVEY.md §8b; traffic
 * n (old_w + new_w) / 8 bytes per segment, §8d).  The reference's BitCompressFromSuccinct
 * (column_segment.cpp:348-383) re-packs in place from full-width slots; here the source is any encoded form
 * (padded, wider than needed after the value range shrank, or unpacked slots) and the destination is a second
 * layout over the SAME segments (type, counts, value offsets), out of place:
 *   adac_analyze_packed  min/max of the decoded values under `rule`, left in dst for adac_plan(dst, ...);
 *   adac_repack          decode at src's width/min, subtract dst's min, pack at dst's width into d_dst_words;
 *   adac_reencode        analyze_packed + adac_plan(dst) + repack.
 * The result is bit-identical to adac_encode of the decoded values.  d_validity as for adac_analyze / adac_pack. */
adac_status adac_analyze_packed(adac_layout *src, const uint64_t *d_src_words, const uint64_t *d_validity, int rule,
                                adac_layout *dst);
adac_status adac_repack(adac_layout *src, const uint64_t *d_src_words, const uint64_t *d_validity, adac_layout *dst,
                        uint64_t *d_dst_words);
adac_status adac_reencode(adac_layout *src, const uint64_t *d_src_words, const uint64_t *d_validity, int rule,
                          int pad_to_byte, adac_layout *dst, uint64_t *d_dst_words);

/* Decode every segment: out[val_off + i] = T(read_int(words, i*w, w) + min).  Replaces SuccinctScanPartial
 * over a whole column (succinct.cpp:123-144) and ColumnSegment::UncompressSuccinct (column_segment.cpp:458-506).
 * Unpacked segments are copied without the min add (SURVEY.md §8a parity domain (iii)).
 * d_out must be 16-byte aligned.
 * The decode's work units are cut on 128-byte lines of the output BY ELEMENT INDEX (val_off + row): each unit but a
 * segment's first starts at an element index that is a multiple of 128 / sizeof(T).  That is alignment of the stored
 * addresses, and whole-line stores, when d_out itself is 128-byte aligned, as the blocks of a device allocator are; any
 * 16-byte-aligned d_out decodes to the same values.  adac_layout_ntiles keeps counting the segment-relative tiles. */
adac_status adac_unpack(adac_layout *l, const uint64_t *d_words, void *d_out);

/* Decode `count` values of ONE segment starting at row `start` to d_out[out_off ...]: the scan_vector /
 * scan_partial slots (compression_function.hpp:84-88; succinct.cpp:123-144,232-240). */
adac_status adac_unpack_range(adac_layout *l, const uint64_t *d_words, uint64_t seg, uint64_t start, uint64_t count,
                              void *d_out, uint64_t out_off);

/* The same slots for SEVERAL segments in one launch and WITHOUT a layout: every job names its segment inline (where
 * its words start in d_words, width, min, flags — the fields of adac_segment_desc) and a row range; rows
 * [start, start + count) are decoded to d_out[out_off ...).  The jobs travel in the kernel arguments, so the call
 * allocates nothing and uploads nothing: it is what a host mirror of ColumnData::ScanVector
 * (src/storage/table/column_data.cpp:92-139) uses to serve one vector, and to decode the next few segments of a scan
 * ahead of the consumer.  Any njobs (launched in groups of 48).  out_off * sizeof(T) need not be aligned. */
typedef struct adac_unpack_job {
	uint64_t word_off; /* first uint64 word of the segment in d_words (multiple of 16) */
	uint64_t min;      /* the descriptor's min (ADAC_NO_MIN if none) */
	uint64_t out_off;  /* element offset of the first decoded row in d_out */
	uint32_t start;    /* first row */
	uint32_t count;    /* rows to decode */
	uint8_t width;     /* 1..8*sizeof(T) */
	uint8_t flags;     /* ADAC_SEG_* */
	uint16_t reserved;
	uint32_t reserved2;
} adac_unpack_job;
adac_status adac_unpack_jobs(adac_ctx *ctx, int physical_type, const adac_unpack_job *jobs, uint64_t njobs,
                             const uint64_t *d_words, void *d_out);

/* Point fetch: d_out[k] = value at row d_rows[k] of segment d_segs[k] — the intended semantics of
 * SuccinctFetchRow (succinct.cpp:244-260; the reference implementation ignores row_id). */
adac_status adac_fetch_rows(adac_layout *l, const uint64_t *d_words, const uint32_t *d_segs, const uint32_t *d_rows,
                            uint64_t n, void *d_out);

/* Fused scan + aggregate without materialising: d_sums[seg] = sum of the decoded values, each widened to 64 bits
 * according to T's signedness (sign-extended for the INT types, zero-extended for the UINT types), mod 2^64 —
 * the low 64 bits of SQL SUM over the segment.  (reads packed bytes only.) */
adac_status adac_scan_sum(adac_layout *l, const uint64_t *d_words, uint64_t *d_sums);

/* Fused scan + equality filter: d_counts[seg] = number of rows whose decoded value == key (key given as the
 * bit pattern of T zero-extended) — the `SELECT i FROM t1 WHERE i == k` look-ups of
 * benchmark/micro/succinct/zipf_distribution.cpp:40-48 without materialising the column. */
adac_status adac_scan_count_eq(adac_layout *l, const uint64_t *d_words, uint64_t key, uint64_t *d_counts);

/* Fused scan + range filter: d_counts[seg] = rows with lo <= value <= hi in T's own order (signed for the INT
 * types); lo / hi are bit patterns of T, zero-extended.  With lo = T's minimum or hi = T's maximum this is
 * `<=` / `>=`, with lo == hi it is `==`: the comparison kinds ColumnSegment::FilterSelection pushes down
 * (src/storage/table/column_segment.cpp:575-844).  Evaluated on the packed fields (lo - min, hi - min); a
 * segment whose [min, min + 2^w) cannot intersect the range is skipped without reading it (zonemap skip). */
adac_status adac_scan_count_between(adac_layout *l, const uint64_t *d_words, uint64_t lo, uint64_t hi,
                                    uint64_t *d_counts);

/* Grouped aggregate over TWO packed columns of one table — the shape of TPC-H Q1 on the reference's config 3
 * (`SELECT key, SUM(value), COUNT(*) ... GROUP BY key`, benchmark log TPCH_runtime.txt:2-6; the reference decodes both
 * columns vector by vector, succinct.cpp:123-144, and feeds a hash aggregate).  `values` and `keys` are layouts on the
 * same context with the same row count per segment (types, widths, placements may differ); nothing is materialised.
 * key = the key column's value as an unsigned number of its own width.  d_sums[g], d_counts[g] for g < ngroups are the
 * sum (values widened to 64 bits by the value type's signedness, mod 2^64 — adac_scan_sum's rule) and the number of
 * the rows whose key is g; entry [ngroups] collects the rows whose key is >= ngroups, so both arrays hold ngroups + 1
 * entries.  1 <= ngroups <= 256. */
adac_status adac_scan_group_sum(adac_layout *values, const uint64_t *d_value_words, adac_layout *keys,
                                const uint64_t *d_key_words, uint32_t ngroups, uint64_t *d_sums, uint64_t *d_counts);

/* The same grouped aggregate restricted to the rows whose bit is set in d_validity — Q1's WHERE clause, or a nullable
 * column: `SELECT key, SUM(value), COUNT(*) ... WHERE <filter> GROUP BY key` with the filter evaluated by
 * adac_scan_select_between.  Bit e of word e / 64 of d_validity is element e = val_off + row of the VALUES layout
 * (adac_scan_sum_product's convention); the key layout's value offsets play no part, so a bitmap that
 * adac_scan_select_between wrote on any layout with the values layout's offsets can be passed straight in.
 * A row whose bit is clear contributes to no sum and no count, the overflow entry [ngroups] included: the ngroups + 1
 * counts add up to the number of set bits on rows that segments cover.  Bits that belong to no row (gaps between
 * segments, bits past value_span in the last word) never influence a result, and the call reads no mask word outside
 * the ceil(value_span / 64) words of the values layout.  d_validity == NULL: every row takes part, the result is
 * adac_scan_group_sum's (which is this call with NULL).  Everything else is as there: the same argument checks,
 * d_sums and d_counts (ngroups + 1 entries each) are fully written and need no clearing by the caller, the call
 * enqueues on the context's stream and does not synchronise. */
adac_status adac_scan_group_sum_valid(adac_layout *values, const uint64_t *d_value_words, adac_layout *keys,
                                      const uint64_t *d_key_words, const uint64_t *d_validity, uint32_t ngroups,
                                      uint64_t *d_sums, uint64_t *d_counts);

/* Product aggregate over TWO packed columns of one table — TPC-H Q6's `SUM(l_extendedprice * l_discount) WHERE ...`
 * without materialising either column.  `a` and `b` are layouts on the same context with the same row count per
 * segment (types, widths, placements and encode rules may differ; a == b with the same words gives the sum of squares).
 * d_sums[seg] = sum over the rows of segment seg whose bit is set in d_validity (NULL = every row) of
 * widen(a) * widen(b), mod 2^64.  Each value is widened to 64 bits by its own column's signedness
 * (adac_scan_sum's rule).  The product and the sum are taken mod 2^64.
 * d_validity is indexed in a's element space (a's val_off + row), so a bitmap adac_scan_select_between wrote on a
 * layout with a's value offsets can be passed straight in; b's value offsets play no part.  A segment without rows
 * gets 0; d_sums is fully written by the call. */
adac_status adac_scan_sum_product(adac_layout *a, const uint64_t *d_a_words, adac_layout *b, const uint64_t *d_b_words,
                                  const uint64_t *d_validity, uint64_t *d_sums);

/* Grouped product aggregate over THREE packed columns of one table — TPC-H Q1's
 * `SUM(l_extendedprice * (1 - l_discount)) ... WHERE <filter> GROUP BY l_returnflag, l_linestatus`: with integer
 * decimals it is 100 * SUM(price) - SUM(price * disc) per group, the first term from adac_scan_group_sum_valid, the
 * second from this call.  `a`, `b` and `keys` are layouts on the same context with the same row count per segment
 * (types, widths, placements, encode rules and value offsets may differ; a == b with the same words gives the per-group
 * sum of squares); nothing is materialised.
 * d_sums[g] for g < ngroups = the sum of widen(a) * widen(b) over the rows whose key is g and whose bit is set in
 * d_validity.  Each value is widened to 64 bits by its own column's signedness; the product and the sum are taken mod
 * 2^64 (adac_scan_sum_product's rule).  key = the key column's value as an unsigned number of its own width; rows whose
 * key is >= ngroups go to entry [ngroups]; 1 <= ngroups <= 256 (adac_scan_group_sum's rule).
 * d_validity is indexed in a's element space (a's val_off + row); b's and the key layout's value offsets play no part.
 * NULL = every row.  Bits that belong to no row never influence a result, and the call reads no mask word outside the
 * ceil(value_span(a) / 64) words of a's layout.  A row whose bit is clear contributes to nothing, the overflow entry
 * included.
 * d_counts[g] = the number of contributing rows, as adac_scan_group_sum_valid counts them.  d_counts may be NULL: then
 * no counts are written (Q1 has them from its other aggregates; the fast form then keeps none).
 * d_sums, and d_counts when given, hold ngroups + 1 entries; they are fully written by the call and need no clearing,
 * also when the layouts have no rows.  The call enqueues on the context's stream and synchronises no more than
 * adac_scan_group_sum_valid does.
 * ADAC_ERR_INVALID_ARGUMENT: a NULL layout; layouts on different contexts; per-segment counts that differ between any
 * two of the three layouts; ngroups 0 or > 256; NULL d_sums; a NULL words pointer while there are rows; a words pointer
 * that is not 16-byte aligned.
 * The tuning knob "group_product_rw" (default 1) chooses between the register-walk kernel with the staged kernel for
 * what it leaves, and (0) the staged kernel alone; results never depend on it. */
adac_status adac_scan_group_sum_product(adac_layout *a, const uint64_t *d_a_words, adac_layout *b,
                                        const uint64_t *d_b_words, adac_layout *keys, const uint64_t *d_key_words,
                                        const uint64_t *d_validity, uint32_t ngroups, uint64_t *d_sums,
                                        uint64_t *d_counts);

/* Grouped TRIPLE product aggregate over FOUR packed columns of one table — the term TPC-H Q1's sum_charge adds to the
 * calls above: with integer decimals
 *   SUM(p * (100 - d) * (100 + t)) = 10000 * SUM(p) + 100 * SUM(p * t) - 100 * SUM(p * d) - SUM(p * d * t)   per group,
 * the first term from adac_scan_group_sum_valid, the next two from adac_scan_group_sum_product, the last from this call.
 * Semantics are adac_scan_group_sum_product's with one more factor.  `a`, `b`, `c` and `keys` are layouts on the same
 * context with the same row count per segment (types, widths, placements, encode rules and value offsets may differ);
 * any two or all three of a, b, c may be the same layout with the same words (the per-group sum of cubes, or of
 * a^2 * c); nothing is materialised.
 * d_sums[g] for g < ngroups = the sum of widen(a) * widen(b) * widen(c) over the rows whose key is g and whose bit is
 * set in d_validity.  Each value is widened to 64 bits by its own column's signedness; both multiplications and the sum
 * are taken mod 2^64.  key = the key column's value as an unsigned number of its own width; rows whose key is >= ngroups
 * go to entry [ngroups]; 1 <= ngroups <= 256.
 * d_validity is indexed in a's element space (a's val_off + row); the value offsets of b, c and keys play no part.
 * NULL = every row.  Bits that belong to no row never influence a result, and the call reads no mask word outside the
 * ceil(value_span(a) / 64) words of a's layout.  A row whose bit is clear contributes to nothing, the overflow entry
 * included.
 * d_counts[g] = the number of contributing rows; d_counts may be NULL: then no counts are written.
 * d_sums, and d_counts when given, hold ngroups + 1 entries; they are fully written by the call and need no clearing,
 * also when the layouts have no rows.  The call enqueues on the context's stream and synchronises no more than
 * adac_scan_group_sum_product does.  The partial buffer, the call counter and the hand-over slots are a's, shared with
 * adac_scan_group_sum[_valid] and adac_scan_group_sum_product: the entry points may be called in any order on one layout.
 * ADAC_ERR_INVALID_ARGUMENT: a NULL layout; layouts on different contexts; per-segment counts that differ between any
 * two of the four layouts; ngroups 0 or > 256; NULL d_sums; a NULL words pointer while there are rows; a words pointer
 * that is not 16-byte aligned.
 * The tuning knob "group_product3_rw" (default 1) chooses between the register-walk kernel with the staged kernel for
 * what it leaves, and (0) the staged kernel alone; results never depend on it. */
adac_status adac_scan_group_sum_product3(adac_layout *a, const uint64_t *d_a_words, adac_layout *b,
                                         const uint64_t *d_b_words, adac_layout *c, const uint64_t *d_c_words,
                                         adac_layout *keys, const uint64_t *d_key_words, const uint64_t *d_validity,
                                         uint32_t ngroups, uint64_t *d_sums, uint64_t *d_counts);

/* All of TPC-H Q1's grouped sums in ONE scan over FIVE packed columns of one table — what the three
 * adac_scan_group_sum_valid, two adac_scan_group_sum_product and one adac_scan_group_sum_product3 calls of the plan above
 * return, with every column, the keys and the mask read once.  In Q1 a = l_extendedprice, b = l_discount, c = l_tax,
 * q = l_quantity.  `a`, `b`, `c`, `q` and `keys` are layouts on the same context with the same row count per segment
 * (types, widths, placements, encode rules and value offsets may differ); any of a, b, c, q may be the same layout with
 * the same words; nothing is materialised.
 * d_out holds ADAC_Q1_TERMS * (ngroups + 1) words: term t of group g is d_out[t * (ngroups + 1) + g], over the rows whose
 * key is g and whose bit is set in d_validity:
 *   ADAC_Q1_COUNT    the number of those rows           (adac_scan_group_sum_valid's d_counts)
 *   ADAC_Q1_SUM_Q    the sum of widen(q)                (adac_scan_group_sum_valid on q)
 *   ADAC_Q1_SUM_A    the sum of widen(a)                (... on a)
 *   ADAC_Q1_SUM_B    the sum of widen(b)                (... on b)
 *   ADAC_Q1_SUM_AB   the sum of widen(a) * widen(b)     (adac_scan_group_sum_product on a, b)
 *   ADAC_Q1_SUM_AC   the sum of widen(a) * widen(c)     (... on a, c)
 *   ADAC_Q1_SUM_ABC  the sum of widen(a) * widen(b) * widen(c)   (adac_scan_group_sum_product3)
 * Each value is widened to 64 bits by its own column's signedness; products and sums are taken mod 2^64.  key = the key
 * column's value as an unsigned number of its own width; rows whose key is >= ngroups go to entry [ngroups];
 * 1 <= ngroups <= 256.
 * d_validity is indexed in a's element space (a's val_off + row); the value offsets of b, c, q and keys play no part.
 * NULL = every row.  Bits that belong to no row never influence a result, and the call reads no mask word outside the
 * ceil(value_span(a) / 64) words of a's layout.  A row whose bit is clear contributes to no term, COUNT and the overflow
 * entry included.
 * d_out is fully written by the call and needs no clearing, also when the layouts have no rows.  The call enqueues on
 * the context's stream and synchronises no more than adac_scan_group_sum_product3 does.  The partial buffer, the call
 * counter and the hand-over slots are a's, shared with the other grouped scans: the entry points may be called in any
 * order on one layout.
 * ADAC_ERR_INVALID_ARGUMENT: a NULL layout; layouts on different contexts; per-segment counts that differ between any
 * two of the five layouts; ngroups 0 or > 256; NULL d_out; a NULL words pointer while there are rows; a words pointer
 * that is not 16-byte aligned.
 * The tuning knob "group_q1_rw" (default 1) chooses between the register-walk kernel with the staged kernel for what it
 * leaves, and (0) the staged kernel alone; results never depend on it. */
#define ADAC_Q1_TERMS 7
enum { ADAC_Q1_COUNT = 0, ADAC_Q1_SUM_Q = 1, ADAC_Q1_SUM_A = 2, ADAC_Q1_SUM_B = 3,
       ADAC_Q1_SUM_AB = 4, ADAC_Q1_SUM_AC = 5, ADAC_Q1_SUM_ABC = 6 };
adac_status adac_scan_group_sum_q1(adac_layout *a, const uint64_t *d_a_words, adac_layout *b, const uint64_t *d_b_words,
                                   adac_layout *c, const uint64_t *d_c_words, adac_layout *q, const uint64_t *d_q_words,
                                   adac_layout *keys, const uint64_t *d_key_words, const uint64_t *d_validity,
                                   uint32_t ngroups, uint64_t *d_out);

/* Diagnostic, not part of the drop-in boundary: *left = the number of scan groups of `l` that the register-walk kernel of
 * the layout's LAST grouped scan (adac_scan_group_sum, adac_scan_group_sum_valid, adac_scan_group_sum_product,
 * adac_scan_group_sum_product3 or adac_scan_group_sum_q1 with `l` as the value / `a` layout) left to the staged kernel; 0 when the walk took every group, when it was not launched (more
 * than 8 bins, or its knob at 0: the staged kernel then takes everything) or when no grouped scan ran.  Synchronises the
 * context's stream.  The tests hold the kernels' choice of form against the host mirror of the rule with it. */
adac_status adac_debug_group_handover(adac_layout *l, uint64_t *left);

/* The same two scans with a DuckDB validity mask over the element index space (bit e of word e/64 set = row e
 * valid, as for adac_analyze): NULL rows take no part in the aggregate — what SUM / COUNT over a nullable
 * column mean.  d_validity == NULL is the unmasked scan. */
adac_status adac_scan_sum_valid(adac_layout *l, const uint64_t *d_words, const uint64_t *d_validity, uint64_t *d_sums);
adac_status adac_scan_count_between_valid(adac_layout *l, const uint64_t *d_words, const uint64_t *d_validity,
                                          uint64_t lo, uint64_t hi, uint64_t *d_counts);

/* Filter push-down with a selection result — ColumnSegment::FilterSelection (column_segment.cpp:575-844) on the
 * packed bytes: bit e of d_bitmap (element index e = val_off + row, the same index space as the validity mask) is
 * set iff the row is valid (d_validity, NULL = every row) and lo <= value <= hi in T's own order; d_counts[seg] =
 * rows selected.  d_bitmap has ceil(value_span / 64) words, is cleared by the call and must not alias
 * d_validity.  Because the result has the validity mask's layout it can be handed to the next column's scan
 * (adac_scan_select_between again for a conjunction, adac_scan_sum_valid / adac_scan_count_between_valid for the
 * aggregate) when the columns share their value offsets: a multi-column filter + aggregate (TPC-H Q6's shape)
 * that never materialises a value. */
adac_status adac_scan_select_between(adac_layout *l, const uint64_t *d_words, const uint64_t *d_validity, uint64_t lo,
                                     uint64_t hi, uint64_t *d_bitmap, uint64_t *d_counts);

/* Filter push-down with a predicate between TWO columns of a row — TPC-H Q12's `l_commitdate < l_receiptdate`, Q4,
 * Q21, or a plain `a = b` — on the packed bytes of both: select the rows where value(a) <cmp> value(b).
 * adac_scan_sum_product's pair rules hold: `a` and `b` are layouts on one context with the same row count per segment;
 * types, widths, placements, encode rules and value offsets may differ.  a == b with the same words is legal: EQ then
 * selects every wanted row, LT and GT none.
 * cmp: an OR of ADAC_CMP_LT / ADAC_CMP_EQ / ADAC_CMP_GT (declared with adac_bp_scan_select_compare below), 1 ... 6.
 * A row is selected iff its bit is set in d_validity (a's element space, a's val_off + row; NULL: every row) and the
 * comparison holds for the values adac_unpack would write for the two columns.  The values compare as mathematical
 * integers: each is widened by its own column's signedness, and a negative value of a signed column is smaller than
 * every value of an unsigned one; int64 against uint64 is exact.
 * d_counts[seg] = rows selected, over a's nseg words, written for segments without rows too.
 * d_bitmap: ceil(value_span(a) / 64) words, fully written by the call: bits of elements that no segment covers are
 * zero, nothing is pre-cleared by the caller.  It must not alias d_validity.  Like adac_scan_select_between's result
 * it is usable as the d_validity of every other scan on a layout with a's value offsets.  No mask word outside
 * ceil(value_span(a) / 64) is read.
 * ADAC_ERR_INVALID_ARGUMENT, on the host before anything is enqueued: a NULL layout; layouts on different contexts;
 * per-segment counts that differ; cmp 0 or above 6; NULL d_counts while a has segments; a NULL or not 16-byte aligned
 * words pointer while there are rows; for the select form NULL d_bitmap while value_span(a) != 0, or
 * d_bitmap == d_validity.
 * Both calls enqueue on the context's stream and synchronise no more than adac_scan_sum_product does.
 * A scan group (some consecutive tiles of one segment) in which both segments are packed against a frame of reference
 * that stays inside the type, so that [frame, frame + 2^width - 1] is known for each, and the two intervals are
 * disjoint, is decided from the two descriptors: no packed word of either column is read (sorted or clustered dates). */
adac_status adac_scan_select_compare(adac_layout *a, const uint64_t *d_a_words, adac_layout *b,
                                     const uint64_t *d_b_words, const uint64_t *d_validity, uint32_t cmp,
                                     uint64_t *d_bitmap, uint64_t *d_counts);
/* the counts alone: no bitmap is written */
adac_status adac_scan_count_compare(adac_layout *a, const uint64_t *d_a_words, adac_layout *b,
                                    const uint64_t *d_b_words, const uint64_t *d_validity, uint32_t cmp,
                                    uint64_t *d_counts);

/* Filter push-down against a BIT SET INDEXED BY VALUE, and the scan that builds such a set: an IN list (TPC-H Q12's
 * l_shipmode IN ('MAIL', 'SHIP'), Q16, Q19) and the two sides of a semi-join on a dense integer key (Q4's EXISTS:
 * adac_scan_select_compare on the lineitem dates, adac_scan_build_member over l_orderkey under that bitmap,
 * adac_scan_select_member over o_orderkey, adac_scan_group_sum_valid for the counts) on the packed bytes.
 * The set covers the values [set_base, set_base + set_bits - 1] in T's own order; set_base is a bit pattern of T,
 * zero-extended (adac_scan_select_between's convention for lo).  d_set has ceil(set_bits / 64) words; bit i of word
 * i / 64 stands for the value set_base + i.  The index of a value v is t = (bits(v) ^ sbit) - (bits(set_base) ^ sbit) in
 * 64-bit unsigned arithmetic, sbit the sign bit of a signed T and 0 otherwise; v is in the domain iff t < set_bits.
 * Probe (select / count): a row is selected iff its bit is set in d_validity (element space, val_off + row; NULL: every
 * row), its value — the one adac_unpack would write — is in the domain and its set bit is 1.  Bits of the last set word
 * at positions >= set_bits are never treated as members, whatever they hold.  d_bitmap and d_counts follow
 * adac_scan_select_compare's rules: both fully written by the call, bits of uncovered elements zero, the result usable
 * as any other scan's d_validity, no mask word outside ceil(value_span / 64) read.
 * Build: d_set is fully written by the call (the caller clears nothing; bits >= set_bits of the last word end up zero):
 * bit t is set iff some wanted row (d_validity as above) has a value in the domain with index t; wanted rows outside the
 * domain are ignored.  d_counts[seg] = the wanted rows of the segment whose value lies in the domain (rows, not distinct
 * values); segments without rows get 0.
 * ADAC_ERR_INVALID_ARGUMENT, on the host before anything is enqueued: set_bits outside 1 ... 2^32; a domain that leaves
 * the type (set_base with bits above the type, or set_base + set_bits - 1 past T's maximum in T's order); a NULL layout;
 * NULL d_counts while the layout has segments; NULL d_set; a NULL or not 16-byte aligned words pointer while there are
 * rows; for the select form NULL d_bitmap while value_span != 0, or d_bitmap == d_validity; d_set overlapping d_bitmap
 * or d_validity.  A layout without segments returns ADAC_OK without touching the device (the build then writes no set).
 * All three calls enqueue on the context's stream and synchronise no more than adac_scan_select_compare does.
 * A scan group whose segment is packed against a frame of reference that stays inside the type, with
 * [frame, frame + 2^width - 1] apart from the domain, is decided from the descriptor: no packed word and no set word is
 * read (the zonemap skip of a join filter).  A segment whose interval reaches at most 65536 bits of the set (every width
 * up to 16) works on a copy of that window in on-chip memory. */
adac_status adac_scan_select_member(adac_layout *l, const uint64_t *d_words, const uint64_t *d_validity,
                                    const uint64_t *d_set, uint64_t set_base, uint64_t set_bits, uint64_t *d_bitmap,
                                    uint64_t *d_counts);
/* the counts alone: no bitmap is written */
adac_status adac_scan_count_member(adac_layout *l, const uint64_t *d_words, const uint64_t *d_validity,
                                   const uint64_t *d_set, uint64_t set_base, uint64_t set_bits, uint64_t *d_counts);
adac_status adac_scan_build_member(adac_layout *l, const uint64_t *d_words, const uint64_t *d_validity,
                                   uint64_t set_base, uint64_t set_bits, uint64_t *d_set, uint64_t *d_counts);

/* SUM(value), COUNT(*) GROUP BY a DENSE INTEGER KEY of any cardinality — TPC-H Q18's SUM(l_quantity) GROUP BY
 * l_orderkey, Q13's COUNT(*) GROUP BY o_custkey, Q3 / Q10's revenue per order or customer, any GROUP BY on a date — on
 * the packed bytes of both columns, without a hash table: the results are arrays indexed by the key.  Called on the KEY
 * layout.  The domain is [key_base, key_base + key_span - 1] in the key type's own order, key_base a bit pattern of the
 * key type, zero-extended, 1 <= key_span <= 2^32, the domain inside the type: adac_scan_build_member's rule.  A key's
 * index is the member scans' t = (bits(k) ^ sbit) - (bits(key_base) ^ sbit); the key is in the domain iff t < key_span.
 * A row is wanted iff its bit is set in d_validity, indexed in the KEYS' element space (the keys' val_off + row; NULL:
 * every row); the value layout's offsets play no part.  Bits of elements that no segment covers never influence a
 * result, no mask word outside ceil(value_span(keys) / 64) is read, and a bitmap that any select scan wrote on a layout
 * with the keys' offsets passes straight in.
 * d_sums[t] = the sum of widen(value) mod 2^64 over the wanted rows whose key has index t, each value widened by the
 * value column's own signedness (adac_scan_sum's rule); d_counts[t] = the number of those rows.  Both hold key_span
 * words and are fully written by the call: the caller clears nothing.  d_counts may be NULL in the sum entry.
 * d_seg_rows[seg] = the wanted rows of the segment whose key lies in the domain (adac_scan_build_member's d_counts):
 * nseg words, written for segments without rows too; may be NULL.  Wanted rows with a key outside the domain contribute
 * nowhere.  Because d_sums is a dense uint64 array indexed by key, adac_encode + adac_scan_select_between over it give a
 * bitmap that is bit for bit a member set over the same domain: the d_set of adac_scan_select_member on the other
 * table's key (Q18's HAVING SUM(l_quantity) > 300, then the orders).
 * adac_scan_sum_product's pair rules hold: one context for both layouts and the same row count per segment; types,
 * widths, placements, encode rules and value offsets may differ; values == keys with the same words is legal.
 * ADAC_ERR_INVALID_ARGUMENT, on the host before anything is enqueued (the call then writes nothing): a NULL layout;
 * layouts on different contexts; per-segment counts that differ; key_span outside 1 ... 2^32 or a domain that leaves the
 * type; NULL d_sums (sum entry) or NULL d_counts (count entry); a NULL or not 16-byte aligned words pointer while there
 * are rows; any two of d_sums, d_counts, d_seg_rows, d_validity overlapping.  A key layout without segments returns
 * ADAC_OK and still zero-fills d_sums and d_counts: their size comes from key_span.
 * Both calls enqueue on the context's stream and synchronise no more than adac_scan_build_member does.
 * A scan group whose key segment is packed against a frame of reference that stays inside the type, with
 * [frame, frame + 2^width - 1] apart from the domain, is decided from the descriptor: no packed word of either column
 * and no mask word is read.  A key segment whose interval reaches at most 512 indices adds up in on-chip memory.  A
 * lane adds up each run of equal keys among its consecutive rows before it touches memory (sorted keys: one atomic per
 * run, not per row); the tuning knob "group_dense_combine" 0 turns that off, results never depend on it. */
adac_status adac_scan_group_sum_dense(adac_layout *keys, const uint64_t *d_key_words, adac_layout *values,
                                      const uint64_t *d_value_words, const uint64_t *d_validity, uint64_t key_base,
                                      uint64_t key_span, uint64_t *d_sums, uint64_t *d_counts, uint64_t *d_seg_rows);
/* the counts alone: no value column is read */
adac_status adac_scan_group_count_dense(adac_layout *keys, const uint64_t *d_key_words, const uint64_t *d_validity,
                                        uint64_t key_base, uint64_t key_span, uint64_t *d_counts, uint64_t *d_seg_rows);

/* SUM(value), COUNT(*) GROUP BY A CODE LOOKED UP THROUGH A DENSE KEY — the star-join aggregate: TPC-H Q5 / Q7 / Q8 / Q9's
 * revenue by the nation of the supplier behind l_suppkey, Q10 / Q3 by an attribute of the customer or order behind
 * o_custkey / l_orderkey, Q14 / Q19 by an attribute of the part behind l_partkey — on the packed bytes of both columns,
 * without a hash table, a materialised code column or a global atomic per row.  Called on the KEY layout.
 * Domain and mask: the domain [key_base, key_base + key_span - 1], a key's index t = (bits(k) ^ sbit) - (bits(key_base)
 * ^ sbit), "in the domain iff t < key_span" and the check that the domain stays inside the key type are exactly
 * adac_scan_group_sum_dense's; 1 <= key_span <= 2^32.  A row is wanted iff its bit is set in d_validity, indexed in the
 * KEYS' element space (NULL: every row); bits of elements that no segment covers never influence a result and no mask
 * word outside ceil(value_span(keys) / 64) is read.
 * The map: d_map holds one byte per index of the domain, in an allocation of key_span rounded up to a multiple of 8
 * bytes, 8-byte aligned (the member set's word rule).  Bytes at indices >= key_span may hold anything and never influence
 * a result; no byte outside that allocation is read; a byte is read only at an index some wanted row inside the domain
 * has, or as part of an on-chip copy of the window a segment can reach.
 * Probe (sum / count): a wanted row whose key has index t in the domain has group g = d_map[t]; it adds widen(value) (the
 * value column's own signedness, mod 2^64) to d_sums[min(g, ngroups)] and 1 to d_counts[min(g, ngroups)].  Entry
 * [ngroups] is adac_scan_group_sum's overflow entry: it is how the caller drops the dimension rows a filter removed, by
 * giving them code 255.  1 <= ngroups <= 256.  d_sums and d_counts hold ngroups + 1 words and are fully written by the
 * call: the caller clears nothing.  d_counts may be NULL in the sum entry.  Wanted rows with a key outside the domain
 * contribute nowhere.  d_seg_rows[seg] = the wanted rows of the segment whose key lies in the domain: nseg words, written
 * for segments without rows too; may be NULL.  The ngroups + 1 counts add up to the sum of d_seg_rows.
 * adac_scan_sum_product's pair rules hold: one context for both layouts and the same row count per segment; types,
 * widths, placements, encode rules and value offsets may differ; values == keys with the same words is legal.
 * ADAC_ERR_INVALID_ARGUMENT, on the host before anything is enqueued (the call then writes nothing): a NULL layout;
 * layouts on different contexts; per-segment counts that differ; key_span outside 1 ... 2^32 or a domain that leaves the
 * type; ngroups outside 1 ... 256; NULL d_map or d_map not 8-byte aligned; NULL d_sums (sum entry) or NULL d_counts
 * (count entry); a NULL or not 16-byte aligned words pointer while there are rows; any two of d_sums, d_counts,
 * d_seg_rows, d_validity overlapping; d_map overlapping d_sums, d_counts or d_seg_rows.  A key layout without segments
 * returns ADAC_OK and still zero-fills d_sums and d_counts.
 * Both calls enqueue on the context's stream and synchronise no more than adac_scan_group_sum_dense does.
 * A scan group whose key segment is packed against a frame of reference that stays inside the type, with
 * [frame, frame + 2^width - 1] apart from the domain, is decided from the descriptor: no packed word of either column,
 * no mask word and no map byte is read.  A key segment whose interval reaches at most 2048 indices (every width up to
 * 11, every domain of at most 2048 keys) looks its rows up in an on-chip copy of that window of the map.  Rows of the
 * groups below ngroups add up in replicated on-chip bins, rows of the overflow entry in registers; the tuning knob
 * "group_mapped_copies" (0 = as many copies as fit, n = at most n) never changes a result. */
adac_status adac_scan_group_sum_mapped(adac_layout *keys, const uint64_t *d_key_words, adac_layout *values,
                                       const uint64_t *d_value_words, const uint64_t *d_validity, const uint8_t *d_map,
                                       uint64_t key_base, uint64_t key_span, uint32_t ngroups, uint64_t *d_sums,
                                       uint64_t *d_counts, uint64_t *d_seg_rows);
/* the counts alone: no value column is read */
adac_status adac_scan_group_count_mapped(adac_layout *keys, const uint64_t *d_key_words, const uint64_t *d_validity,
                                         const uint8_t *d_map, uint64_t key_base, uint64_t key_span, uint32_t ngroups,
                                         uint64_t *d_counts, uint64_t *d_seg_rows);
/* the build side: d_map[key - key_base] = code of that row.  `keys` and `codes` are two columns of the dimension table
 * (the pair rules above); domain, mask and d_seg_rows as above.  d_map (the rounded-up allocation, pad bytes included)
 * is fully written by the call: every byte is `fill` (0 ... 255), except that for each wanted row of `keys` whose key is
 * in the domain d_map[t] = min(code, 255), the code being the `codes` column's value as an unsigned number of its own
 * width (adac_scan_group_sum's key rule: a negative code of a signed type saturates).  If several wanted rows share an
 * index and disagree on the code, the entry holds one of their codes, unspecified which; primary keys never do.
 * ADAC_ERR_INVALID_ARGUMENT as above, with fill above 255 and d_map overlapping d_seg_rows or d_validity; a key layout
 * without segments still fills d_map.  For a dimension whose key is dense in row order (supplier, customer, part)
 * adac_unpack of a uint8 code column already IS the map, with key_base the first key: no build is needed. */
adac_status adac_scan_build_map(adac_layout *keys, const uint64_t *d_key_words, adac_layout *codes,
                                const uint64_t *d_code_words, const uint64_t *d_validity, uint64_t key_base,
                                uint64_t key_span, uint32_t fill, uint8_t *d_map, uint64_t *d_seg_rows);

/* SUM(a * b), SUM(a), COUNT(*) GROUP BY A CODE LOOKED UP THROUGH A DENSE KEY, from one scan of three packed columns of
 * one table — what TPC-H's revenue, SUM(l_extendedprice * (1 - l_discount)), needs per group in Q5 / Q7 / Q8 / Q9 / Q10 /
 * Q3 / Q14 / Q19.  Recipe for Q5 with integer decimals (price in cents, discount in hundredths): keys = l_suppkey,
 * a = l_extendedprice, b = l_discount, d_map = the supplier's nation (255 for suppliers the region filter drops); then
 *     revenue[g] = 100 * d_sums_a[g] - d_sums_ab[g]      (mod 2^64, in units of 1/10000)
 * for g < ngroups, and entry [ngroups] holds what the filter removed.  Called on the KEY layout.
 * Domain, index, mask and map are exactly adac_scan_group_sum_mapped's: the domain [key_base, key_base + key_span - 1],
 * t = (bits(k) ^ sbit) - (bits(key_base) ^ sbit), "in the domain iff t < key_span", 1 <= key_span <= 2^32, the domain
 * inside the key type; d_validity indexed in the KEYS' element space (NULL: every row), no mask word outside
 * ceil(value_span(keys) / 64) read, bits of uncovered elements never matter; d_map one byte per index in an allocation
 * of key_span rounded up to a multiple of 8 bytes, 8-byte aligned, pad bytes and bytes at indices >= key_span never
 * influence a result, no byte outside the allocation is read.
 * Contributions: a wanted row inside the domain with g = d_map[t] adds widen(a) * widen(b) to d_sums_ab[min(g, ngroups)],
 * widen(a) to d_sums_a[min(g, ngroups)] and 1 to d_counts[min(g, ngroups)].  Each factor is widened to 64 bits by its own
 * column's signedness; the product and the sums are taken mod 2^64 (adac_scan_sum_product's rule).  1 <= ngroups <= 256.
 * The three arrays hold ngroups + 1 words and are fully written by the call: the caller clears nothing.  d_sums_a and
 * d_counts may each be NULL; d_sums_ab may not.  d_seg_rows (nseg words, may be NULL) as in adac_scan_group_sum_mapped.
 * Pair rules: a, b and keys are on one context with the same row count per segment; types, widths, placements, encode
 * rules and value offsets may differ.  a == b with the same words is legal (the per-code sum of squares); a or b may be
 * the key layout itself.
 * ADAC_ERR_INVALID_ARGUMENT, on the host before anything is enqueued (the call then writes nothing): a NULL layout (any
 * of the three); layouts on different contexts; per-segment counts that differ between any two of them; key_span outside
 * 1 ... 2^32 or a domain that leaves the type; ngroups outside 1 ... 256; NULL d_map or d_map not 8-byte aligned; NULL
 * d_sums_ab; a NULL or not 16-byte aligned words pointer of any of the three columns while there are rows; any two of
 * d_sums_ab, d_sums_a, d_counts, d_seg_rows, d_validity overlapping; d_map overlapping d_sums_ab, d_sums_a, d_counts or
 * d_seg_rows.  A key layout without segments returns ADAC_OK and still zero-fills the outputs that were given.
 * The call enqueues on the context's stream and synchronises no more than adac_scan_group_sum_mapped does.
 * A scan group whose key segment is packed against a frame of reference that stays inside the type, with
 * [frame, frame + 2^width - 1] apart from the domain, is decided from the descriptor: no packed word of any of the three
 * columns, no mask word and no map byte is read.  The on-chip window of the map (2048 indices) and the replicated
 * on-chip bins are adac_scan_group_sum_mapped's; the tuning knob "group_mapped_copies" applies here too and never
 * changes a result.  a and b are read in registers-and-LDS form while both are at most 32 bits wide and packed against
 * a frame that stays inside their types; any other segment takes a slower staged reader with the same results. */
adac_status adac_scan_group_sum_product_mapped(adac_layout *keys, const uint64_t *d_key_words, adac_layout *a,
                                               const uint64_t *d_a_words, adac_layout *b, const uint64_t *d_b_words,
                                               const uint64_t *d_validity, const uint8_t *d_map, uint64_t key_base,
                                               uint64_t key_span, uint32_t ngroups, uint64_t *d_sums_ab,
                                               uint64_t *d_sums_a, uint64_t *d_counts, uint64_t *d_seg_rows);

/* Materialise only the selected rows: d_out receives, densely and in row order (segment by segment), the values of
 * the rows whose bit is set in d_bitmap (the result of adac_scan_select_between, or any mask over the element index
 * space); d_out_ids, if not NULL, receives their element indices (val_off + row).  *total_out, if not NULL, is set
 * to the number of rows written (this makes the call synchronous); d_out must hold at least that many values —
 * the sum of the select's d_counts, or total_values in the worst case.  The scan-with-selection half of
 * ColumnSegment::FilterSelection (column_segment.cpp:575-844): a tile is decoded once, rows that did not pass are
 * never written. */
adac_status adac_unpack_selected(adac_layout *l, const uint64_t *d_words, const uint64_t *d_bitmap, void *d_out,
                                 uint64_t *d_out_ids, uint64_t *total_out);

/* ---------------------------------------------------------------------------------------------
 * Persistence in HBM: the block images of MANY packed segments built / parsed by one kernel, so
 * that a checkpoint is one device pass + one device-to-host copy (and a load one host-to-device copy + one pass)
 * instead of a copy per segment.  This is the ConvertToPersistent the reference leaves empty for SUCCINCT
 * (src/storage/table/column_segment.cpp:529-533; the checkpoint-side Compress / FinalizeCompress slots,
 * src/storage/compression/succinct.cpp:91-119, never reach a block).  descs[i]: the segment (word_off into d_words,
 * count, width, min, flags); block_offs[i]: byte offset (multiple of 8) of its image in d_blocks, which spans
 * adac_block_stride(count, width) bytes; the first adac_block_bytes of them are exactly what adac_block_write
 * produces (sdsl::int_vector<0>::serialize + trailer).  Both calls synchronise the stream.
 * adac_blocks_read also zeroes the segment's arena words past its packed words and returns
 * ADAC_ERR_INVALID_ARGUMENT when an image's header does not match its descriptor (build descs with adac_block_peek).
 * ------------------------------------------------------------------------------------------- */
adac_status adac_blocks_write(adac_ctx *ctx, int physical_type, const adac_segment_desc *descs,
                              const uint64_t *block_offs, uint64_t nseg, const uint64_t *d_words, void *d_blocks);
adac_status adac_blocks_read(adac_ctx *ctx, int physical_type, const adac_segment_desc *descs,
                             const uint64_t *block_offs, uint64_t nseg, const void *d_blocks, uint64_t *d_words);

/* ---------------------------------------------------------------------------------------------
 * DuckDB BITPACKING segments — the persistent counterpart of the succinct codec: decode, fused
 * filter / aggregate scans (adac_bp_scan_*) and compress.
 * A segment is the block image DuckDB's checkpoint writes (src/storage/compression/bitpacking.cpp:357-538):
 * metadata groups of 2048 rows in CONSTANT / CONSTANT_DELTA / DELTA_FOR / FOR mode, packed with fastpforlib.
 * Replaces BitpackingScanPartial / BitpackingScan (:736-826) and BitpackingFetchRow (:827-870).
 * ------------------------------------------------------------------------------------------- */
typedef struct adac_bp_layout adac_bp_layout;

/* block_offs[i]: byte offset (multiple of 16) of segment i's block inside the device buffer handed to the scan
 * calls — blocks must be followed by at least 16 readable bytes (a whole Storage::BLOCK_SIZE image is);
 * counts[i]: rows of segment i; out_offs[i]: element offset of its first row in the output, NULL = back to back. */
adac_status adac_bp_layout_create(adac_ctx *ctx, int physical_type, const uint64_t *block_offs, const uint32_t *counts,
                                  const uint64_t *out_offs, uint64_t nseg, adac_bp_layout **out);
void adac_bp_layout_destroy(adac_bp_layout *l);
uint64_t adac_bp_layout_ngroups(const adac_bp_layout *l);
uint64_t adac_bp_layout_total_values(const adac_bp_layout *l);
/* elements an output / validity mask / bitmap over this layout spans: max(out_off + count) */
uint64_t adac_bp_layout_value_span(const adac_bp_layout *l);
/* Parse every group's header (mode, width, frame of reference, payload position) out of the block images into
 * the layout's device table — the analogue of BitpackingScanState::LoadNextGroup (bitpacking.cpp:597-640) for all
 * groups at once.  adac_bp_unpack binds by itself when handed a different buffer; call this again after
 * rewriting blocks in place. */
adac_status adac_bp_bind(adac_bp_layout *l, const void *d_blocks);
/* Full scan: every row of every segment to d_out (16-byte aligned), one workgroup per 2048-row metadata group. */
adac_status adac_bp_unpack(adac_bp_layout *l, const void *d_blocks, void *d_out);
/* Rows [start, start + count) of segment `seg` into d_out[out_off ...] — BitpackingScanPartial / BitpackingScan
 * (bitpacking.cpp:736-826) for any start: a DELTA_FOR group that the range enters in the middle is prefix-summed
 * from its first row, as the reference's Skip + LoadNextGroup do. */
adac_status adac_bp_unpack_range(adac_bp_layout *l, const void *d_blocks, uint64_t seg, uint64_t start, uint64_t count,
                                 void *d_out, uint64_t out_off);

/* d_out[k] = row d_rows[k] of segment d_segs[k] */
adac_status adac_bp_fetch_rows(adac_bp_layout *l, const void *d_blocks, const uint32_t *d_segs, const uint32_t *d_rows,
                               uint64_t n, void *d_out);

/* Fused filter / aggregate scans on the block images: nothing is decoded to HBM.  The BITPACKING counterparts of
 * adac_scan_sum_valid / adac_scan_count_between_valid / adac_scan_select_between and of adac_zonemap's typed
 * min / max.  Every result equals the same aggregate taken over what adac_bp_unpack returns for these bytes.
 * Element index space: bit e of d_validity / d_bitmap is element out_offs[seg] + row, where adac_bp_unpack writes
 * that row.  d_validity == NULL: every row; a row whose bit is clear takes no part in any result.
 * All four enqueue on the layout's stream and do not synchronise (they bind like adac_bp_unpack when handed a
 * different buffer); d_sums / d_counts (nseg words), d_minmax (2 * nseg words) and d_bitmap
 * (ceil(value_span / 64) words) are fully written by the call, nothing is pre-cleared by the caller.
 * A CONSTANT or CONSTANT_DELTA group is answered from its header, a FOR group whose [frame, frame + 2^width)
 * interval misses or lies inside [lo, hi] from its header and the mask: no payload byte is read for them. */
/* d_sums[seg] = sum of the values widened to 64 bits by T's signedness, mod 2^64 (adac_scan_sum's rule) */
adac_status adac_bp_scan_sum(adac_bp_layout *l, const void *d_blocks, const uint64_t *d_validity, uint64_t *d_sums);
/* lo / hi: bit patterns of T, zero-extended; lo <= v <= hi in T's own order (signed for the INT types), lo > hi in
 * that order selects nothing (adac_scan_count_between's rule).  d_counts[seg] = rows selected. */
adac_status adac_bp_scan_count_between(adac_bp_layout *l, const void *d_blocks, const uint64_t *d_validity,
                                       uint64_t lo, uint64_t hi, uint64_t *d_counts);
/* + the selection bitmap: bits of elements no segment covers are zero; must not alias d_validity; usable as the
 * d_validity of a second call on a layout with the same out_offs or of a succinct scan sharing the element space.
 * Output ranges of different segments must not overlap. */
adac_status adac_bp_scan_select_between(adac_bp_layout *l, const void *d_blocks, const uint64_t *d_validity,
                                        uint64_t lo, uint64_t hi, uint64_t *d_bitmap, uint64_t *d_counts);
/* d_minmax[2 * seg], d_minmax[2 * seg + 1] = min, max in T's order as bit patterns of T zero-extended; a segment
 * without a selected row reports the empty interval min = T's maximum, max = T's minimum (adac_zonemap's convention) */
adac_status adac_bp_scan_min_max(adac_bp_layout *l, const void *d_blocks, const uint64_t *d_validity,
                                 uint64_t *d_minmax);

/* Pair scans: two BITPACKING columns of the same table walked in step, nothing decoded to HBM.  Both layouts must
 * live on one context and their metadata group tables must agree: the same number of groups, and group i of each
 * with the same element offset and the same row count — else ADAC_ERR_INVALID_ARGUMENT, as for a NULL layout, NULL
 * results, or a blocks pointer that is NULL or not 16-byte aligned while its layout has rows; all checked on the host
 * before anything is enqueued.  Where the SEGMENTS end may differ (a wide column fills its block after 16 groups, a
 * narrow one after 250).  d_validity is indexed in the FIRST layout's element space, out_offs[seg] + row; NULL:
 * every row; no mask word outside that layout's ceil(value_span / 64) words is read.  Both calls enqueue on the
 * context's stream, do not synchronise and bind each layout like adac_bp_unpack when handed a buffer it is not bound
 * to (one layout object passed twice must come with one buffer).  The results are fully written by the call, nothing
 * is pre-cleared by the caller, and equal the same aggregate over what adac_bp_unpack returns for the two buffers. */
/* d_sums[seg], over a's segments (a's nseg words, written for segments without rows too) = sum of widen(a) * widen(b)
 * mod 2^64 over the selected rows, each factor widened by its own type's signedness (adac_scan_sum_product's rule).
 * b's segmentation and out_offs play no part beyond the group check; a == b gives the sum of squares. */
adac_status adac_bp_scan_sum_product(adac_bp_layout *a, const void *d_a_blocks, adac_bp_layout *b, const void *d_b_blocks,
                                     const uint64_t *d_validity, uint64_t *d_sums);
/* SUM(value), COUNT(*) GROUP BY key with adac_scan_group_sum_valid's semantics: key = the key column's value as an
 * unsigned number of its own width (a negative key of a signed type is a large one); rows whose key >= ngroups go
 * to entry [ngroups]; 1 <= ngroups <= 256.  d_sums and d_counts (may be NULL) hold ngroups + 1 words over the whole
 * column, not per segment.  A row whose bit is clear in d_validity (the values layout's element space) contributes
 * to no entry, the overflow entry included.  A group whose key column is CONSTANT (a table sorted by the key)
 * updates its entry once, not once per row. */
adac_status adac_bp_scan_group_sum(adac_bp_layout *values, const void *d_value_blocks, adac_bp_layout *keys,
                                   const void *d_key_blocks, const uint64_t *d_validity, uint32_t ngroups,
                                   uint64_t *d_sums, uint64_t *d_counts);

/* Select the rows where value(a) <cmp> value(b): a predicate between two columns of a row (TPC-H Q12's
 * l_commitdate < l_receiptdate, Q4, Q21, or a = b), evaluated on the block images.  The pair scans' rules above hold:
 * one context, group tables that agree, blocks pointers, binding, enqueue without synchronising.  A row is selected
 * iff its bit is set in d_validity (a's element space, out_offs[seg] + row; NULL: every row) and the comparison holds
 * for the values adac_bp_unpack would write for the two buffers.  The values are compared as mathematical integers,
 * whatever the two types are: each is widened by its own column's signedness, and a negative value of a signed column
 * is smaller than every value of an unsigned one — int32 against int32, uint8 against uint64 and int64 against uint64
 * are all exact.  cmp: an OR of the three bits below, 1 ... 6; 0 or more than 6 is ADAC_ERR_INVALID_ARGUMENT.
 * d_counts[seg] = rows selected, over a's segments (a's nseg words, written for segments without rows too).
 * d_bitmap: ceil(value_span(a) / 64) words, fully written by the call, bits of elements no segment covers zero; must
 * not alias d_validity; usable as the d_validity of any other adac_bp_scan_* call, exactly like
 * adac_bp_scan_select_between's result.  Nothing is pre-cleared by the caller.  a == b with one buffer is legal: EQ
 * then selects every wanted row, LT and GT none.  ADAC_ERR_INVALID_ARGUMENT, on the host before anything is
 * enqueued, beyond the pair scans' checks: cmp out of range; NULL d_counts while a has segments; for the select form
 * NULL d_bitmap while value_span(a) != 0, or d_bitmap == d_validity.
 * A group without a wanted row reads nothing.  A group in which both columns are CONSTANT is decided by one
 * comparison, and one in which each column is CONSTANT or a FOR group whose [frame, frame + 2^width) does not wrap,
 * and the two intervals are disjoint, from the two headers: no payload byte of either column is read. */
enum { ADAC_CMP_LT = 1, ADAC_CMP_EQ = 2, ADAC_CMP_GT = 4 }; /* or-able: LE = 3, NE = 5, GE = 6 */
adac_status adac_bp_scan_select_compare(adac_bp_layout *a, const void *d_a_blocks, adac_bp_layout *b,
                                        const void *d_b_blocks, const uint64_t *d_validity, uint32_t cmp,
                                        uint64_t *d_bitmap, uint64_t *d_counts);
/* the counts alone: no bitmap is written */
adac_status adac_bp_scan_count_compare(adac_bp_layout *a, const void *d_a_blocks, adac_bp_layout *b,
                                       const void *d_b_blocks, const uint64_t *d_validity, uint32_t cmp,
                                       uint64_t *d_counts);

/* Scan with selection on the block images — adac_unpack_selected for BITPACKING, the scan-with-selection half of
 * ColumnSegment::FilterSelection (column_segment.cpp:575-844): d_out receives, densely, as values of the layout's
 * type, the rows whose bit is set in d_bitmap, in group-table order (segment by segment, row order inside a segment);
 * the bit index is element out_offs[seg] + row, the index space of the adac_bp_scan_* calls' d_validity / d_bitmap
 * (the result of adac_bp_scan_select_between, or any mask over it).  The values equal what adac_bp_unpack writes at
 * those elements.  d_out_ids, if not NULL, receives the element indices.  *total_out, if not NULL, is set to the
 * number of rows written, which makes the call synchronous; with total_out == NULL the call only enqueues on the
 * context's stream.  d_out (and d_out_ids) must hold at least that many entries — the sum of the select's d_counts,
 * or total_values in the worst case; nothing is written at or past slot total.  Bits of elements that no segment
 * covers are ignored and no bitmap word outside ceil(value_span / 64) is read.  A metadata group without a selected
 * row reads no payload byte, and a CONSTANT, CONSTANT_DELTA or width-0 group reads none either.  Binds like
 * adac_bp_unpack when handed a buffer the layout is not bound to.  ADAC_ERR_INVALID_ARGUMENT, checked on the host
 * before anything is enqueued: a NULL layout; while the layout has rows, a NULL d_bitmap or d_out, or a d_blocks that
 * is NULL or not 16-byte aligned.  A layout without rows sets *total_out = 0 and writes nothing else. */
adac_status adac_bp_unpack_selected(adac_bp_layout *l, const void *d_blocks, const uint64_t *d_bitmap, void *d_out,
                                    uint64_t *d_out_ids, uint64_t *total_out);

/* Compress side (BitpackingCompress / BitpackingFinalizeCompress, bitpacking.cpp:514-538): per-group statistics
 * on the device, the mode decision of BitpackingState::Flush (:229-294) and the sequential placement of groups
 * into Storage::BLOCK_SIZE blocks (:453-512) on the host, then one device pass writing every group image.
 * force_mode: BitpackingMode (0 AUTO, 1 CONSTANT, 2 CONSTANT_DELTA, 3 DELTA_FOR, 4 FOR — the reference's
 * force_bitpacking_mode).  NULL rows are encoded as the value 0 (the reference leaves them indeterminate). */
typedef struct adac_bp_plan adac_bp_plan;
adac_status adac_bp_plan_create(adac_ctx *ctx, int physical_type, const void *d_vals, const uint64_t *d_validity,
                                uint64_t n, int force_mode, adac_bp_plan **out);
void adac_bp_plan_destroy(adac_bp_plan *p);
/* 0 when some group can be stored in no mode (Flush() == false: BitpackingFinalAnalyze returns INVALID_INDEX) */
int adac_bp_plan_encodable(const adac_bp_plan *p);
uint64_t adac_bp_plan_nseg(const adac_bp_plan *p);
uint64_t adac_bp_plan_groups_by_mode(const adac_bp_plan *p, int mode);
/* first row, row count and used bytes (FlushSegment's total_segment_size) of segment i */
adac_status adac_bp_plan_segment(const adac_bp_plan *p, uint64_t i, uint64_t *start, uint64_t *count,
                                 uint64_t *total_size);
/* Write every segment's block image: segment i at d_blocks + i*block_stride (block_stride >= 262136, multiple of 16).
 * The whole nseg*block_stride range is rewritten (unused bytes zero). */
adac_status adac_bp_write(adac_bp_plan *p, const void *d_vals, const uint64_t *d_validity, void *d_blocks,
                          uint64_t block_stride);

#ifdef __cplusplus
}
#endif
#endif /* ADACODEC_H */
