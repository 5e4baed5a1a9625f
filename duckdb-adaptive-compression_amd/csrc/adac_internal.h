// adac_internal.h — launch wrappers shared between the C ABI (adac_capi.cpp) and the gfx950 kernels
// (adac_kernels.hip).  Not installed; the public surface is include/adacodec.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adacodec.h"
#include "adac_scan_deal.h"
#include "adac_tile_cut.h"

namespace adac {

constexpr int kWorkgroup = 256;       // 4 wavefronts of 64 lanes
constexpr int kTileBytes = 16384;     // decoded bytes per tile: tile = 16 KiB / sizeof(T) values
constexpr uint32_t kNoTile = 0xffffffffu;
constexpr int kLineBytes = 128;       // one cache line of the output: the decode's tiles are cut on them
static_assert(kCutTileBytes == (uint32_t)kTileBytes && kCutLineBytes == (uint32_t)kLineBytes, "adac_tile_cut.h");
static_assert(kDealTileBytes == (uint32_t)kTileBytes, "adac_scan_deal.h");

// TileRef (adac_tile_cut.h): one tile of one segment.  A layout keeps two tables of them: the segment-relative one
// (`first` a multiple of the type's tile size; analyze, pack, the gather, the scan groups, the expanded records) and the
// decode's, cut on lines of the output (cut_tiles_on_lines; adac_unpack only).

// A tile with its segment's CURRENT descriptor folded in (rebuilt whenever descriptors change, like the scan groups): the
// gather (k_gather_c) reads ONE 32-byte record before its first data load instead of the dependent chain tile entry ->
// descriptor — a workgroup's lifetime is a handful of memory round trips, and the bytes a CU keeps in flight per lifetime
// bound that kernel (+4 - 7 %).  The decode (k_unpack) does NOT take it: measured 4 - 17 % slower with the record, same
// box, interleaved (profiles/r03_tile_records.json) — as with the scalar descriptor load of round 3's first session.
struct alignas(32) TileRec {
	uint64_t word_off; // the segment's first word in the arena
	uint64_t elem0;    // element index of the tile's first row
	uint64_t add;      // frame of reference to add back (0 if none)
	uint32_t first;    // first row of the tile inside the segment
	uint16_t n;        // rows in the tile (<= 16384)
	uint8_t width, flags;
};
static_assert(sizeof(TileRec) == 32, "device record");

// ScanGroupRef (adac_scan_deal.h): work item of the fused scans, static per layout and grouping.  ScanGroup is its
// expansion with the segment's current descriptor (rebuilt whenever descriptors change): a scan workgroup then needs ONE
// 64-byte load before its first data load instead of the dependent chain tile entry -> descriptor.
struct alignas(64) ScanGroup {
	adac_segment_desc d;
	uint32_t seg;
	uint32_t first;
	uint32_t n; // rows
	uint32_t seg_groups;
	uint32_t cell_first, cell_last;
	uint16_t n_first, n_last;
	uint32_t pad;
};
static_assert(sizeof(ScanGroup) == 64, "one cache-line record per scan group");

// Single-segment range decode (scan_vector / scan_partial): tiles are implicit.
struct RangeArgs {
	uint32_t seg;
	uint32_t start;
	uint32_t count;
	uint64_t out_off;
};

// Layout-free range decode of several segments in ONE launch (adac_unpack_jobs): the jobs travel by value in the
// kernel-argument segment, so a batch needs no device table, no upload and no allocation — what a host that serves an
// engine vector by vector (or prefetches the next few segments of a scan) can afford per call.
constexpr int kMaxUnpackJobs = 48;
struct UnpackJob {
	uint64_t word_off; // first word of the segment in the arena
	uint64_t add;      // frame of reference to add back (0 if none: unpacked slots, or no min)
	uint64_t out_off;  // element offset of the job's first decoded row in the output
	uint32_t start;    // first row of the segment to decode
	uint32_t count;    // rows to decode
	uint32_t width;
	uint32_t tile0;    // first workgroup of this job in the launch
};
struct UnpackJobTable {
	uint32_t njobs, ntiles;
	UnpackJob jobs[kMaxUnpackJobs];
};
hipError_t launch_unpack_jobs(hipStream_t s, uint32_t type_size, const UnpackJobTable &table, const uint64_t *d_words,
                              void *d_out);

// Launch-shape knobs (adac_set_tuning): which kernel form the scan entry points use and how many persistent
// workgroups are launched.  Defaults are the measured-best settings on MI355X.
struct Tuning {
	int single_pass_encode = 1; // A/B: 0 = analyze + plan + pack as three kernels (the raw column is read twice)
	int group_sum_wide = 0;     // A/B: adac_scan_group_sum always in 64-bit arithmetic
	int group_sum_rw = 1;       // A/B: 0 = adac_scan_group_sum without the register-walk kernel (k_group_sum only)
	int group_product_rw = 1;   // A/B: 0 = adac_scan_group_sum_product without the register-walk kernel (k_group_product only)
	int group_product3_rw = 1;  // A/B: 0 = adac_scan_group_sum_product3 without the register-walk kernel (k_group_product3 only)
	int group_q1_rw = 1;        // A/B: 0 = adac_scan_group_sum_q1 without the register-walk kernel (k_group_q1 only)
	int group_dense_combine = 1; // A/B: 0 = adac_scan_group_sum_dense / _count_dense with one atomic per row (no run combining in the walk)
	int group_dense_window = 1;  // A/B: 0 = the same two without the LDS window (every add goes to global memory)
	int group_mapped_copies = 0; // adac_scan_group_sum_mapped / _count_mapped / _sum_product_mapped: copies of the LDS bins; 0 = as many as fit, n = at most n (1 = one copy)
	int encode_placement = 0;   // single-pass encode: 0 = arena order is segment order (look-back), 1 = order of completion
	int encode_big_image = 1;   // single-pass encode, ordered placement: a segment whose packed words fit the LDS pool is packed there whole and publishes the NEXT footprint before it waits (A/B: 0)
	int encode_publish_ahead = 1; // single-pass encode, ordered placement: the parked flow publishes the NEXT footprint before it waits (A/B: 0)
	int encode_stamps = 0;      // diagnostic: phase time stamps of the single-pass encode (adac_debug_encode_stamps)
	int tile_records = 1;       // expanded 32-byte tile records (TileRec): bit 0 = the gather (k_gather_c: +4 - 7 %), bit 1 = the decode (k_unpack: 4 - 17 % SLOWER, off)
	int scan_cells = 1;         // fused scans: 1 = results (and shared bitmap words) finished inside the scan kernel through arrival cells, 0 = clearing pass + atomics (+ merge kernel)
	int gather_compact = 3;     // adac_unpack_selected: 0 = a store per selected row (k_gather), 1 = wave-level compaction + dense stores (k_gather_c), 3 = the same with non-temporal stores
	int sel_debug = 0;          // diagnostic: selection scan without its flush (1) / without any bitmap emit (2)
	int templated_scan = 1;     // width-templated register path of the fused scans for 4 <= w <= 32
	int scan_tiles_per_wg = 0; // tiles per fused-scan workgroup; 0 = by type (12 tiles of u64, 6 of u32, 8 of u16, 4 of u8)
	int num_cus = 0;        // 0 = the device's own count (256 on a whole MI355X: 8 XCDs x 32 CUs); > 0 overrides
};
extern Tuning g_tuning;

inline uint32_t tile_values(uint32_t type_size) {
	return kTileBytes / type_size;
}
// all-ones mask of a type's width, and its sign bit (0 for the unsigned types)
inline uint64_t type_mask(uint32_t type_size) {
	return type_size >= 8 ? ~0ull : (1ull << (8 * type_size)) - 1ull;
}
inline uint64_t type_sign_bit(uint32_t type_size, bool is_signed) {
	return is_signed ? 1ull << (8 * type_size - 1) : 0ull;
}

// What the launchers take instead of loose parameters.
// A packed column: its type, its segment descriptors and its packed words (BpColumn is the BITPACKING counterpart).
struct Column {
	uint32_t type_size;
	bool is_signed;
	const adac_segment_desc *d_descs;
	const uint64_t *d_words;
};
// The work items of the layout a scan walks, the call's first column: its tiles (the staged kernels') and its scan
// groups (the register-walk kernels' and the per-segment scans', which look at nothing else here).
struct ScanWork {
	const TileRef *d_tiles;
	uint64_t ntiles;
	const ScanGroup *d_scan_groups;
	uint64_t nscan_groups;
};
// The state the grouped scans of one layout share: the partial buffer (group_sum_partial_bytes(), cleared when it is
// allocated) and the number of the call, whose low bit picks the hand-over word.
struct GroupScanState {
	void *d_partial;
	uint32_t call_parity;
};
// The type words every scan kernel takes per column: all-ones mask of the type's width and its sign bit.
struct TypeWords {
	uint64_t tmask, sbit;
};
template <class C> // Column, BpColumn or a layout: anything with type_size and is_signed
inline TypeWords type_words(const C &col) {
	return {type_mask(col.type_size), type_sign_bit(col.type_size, col.is_signed)};
}

// The domain [base, base + span - 1] of a member or dense-key scan in the biased form the kernels work in (MemberDomain,
// adac_scan_member.inl): the key type's words, bits(base) ^ sbit and the span, 1 ... 2^32 with bbase + span - 1 <= tmask.
// The entry points check that rule and make the domain, once per call.
struct KeyDomain {
	uint64_t tmask, sbit, bbase, span;
};
// What every dense-key scan takes: the key column, its layout's work items, the selection (may be null), the domain
// and the rows inside the domain per segment (d_seg_rows, may be null); the caller has cleared every output.
struct DenseScan {
	Column keys;
	ScanWork work;
	const uint64_t *d_validity;
	KeyDomain dom;
	uint64_t *d_seg_rows;
};
// ... and the mapped scans with it: one byte per index of the domain, and the codes they bin (1 ... 256)
struct MappedScan {
	DenseScan scan;
	const uint8_t *d_map;
	uint32_t ngroups;
};

// type_size in {1,2,4,8}; every launcher returns the hipError_t of the launch.
hipError_t launch_analyze(hipStream_t s, uint32_t type_size, bool sign_extend, uint64_t null_bits, int rule,
                          const adac_segment_desc *d_descs, const TileRef *d_tiles, uint64_t ntiles,
                          const void *d_vals, const uint64_t *d_validity, uint64_t *d_minmax);
hipError_t launch_minmax_init(hipStream_t s, uint64_t *d_minmax, uint64_t nseg);
hipError_t launch_plan(hipStream_t s, uint32_t type_size, int rule, int pad_to_byte, adac_segment_desc *d_descs,
                       const uint64_t *d_minmax, uint64_t nseg);
hipError_t launch_pack(hipStream_t s, uint32_t type_size, uint64_t null_bits, const adac_segment_desc *d_descs,
                       const TileRef *d_tiles, uint64_t ntiles, const void *d_vals, const uint64_t *d_validity,
                       uint64_t *d_words);
// decode of a packed column to d_out: every tile (d_recs null: d_tiles is the layout's LINE-CUT table; d_recs the expanded
// records: d_tiles is the segment-relative table they were made from), one range of one segment, and the n rows
// (d_segs[i], d_rows[i])
hipError_t launch_unpack(hipStream_t s, const Column &col, const TileRef *d_tiles, uint64_t ntiles, void *d_out,
                         const TileRec *d_recs);
hipError_t launch_unpack_range(hipStream_t s, const Column &col, RangeArgs range, void *d_out);
hipError_t launch_fetch(hipStream_t s, const Column &col, const uint32_t *d_segs, const uint32_t *d_rows, uint64_t n,
                        void *d_out);
// single-pass encode (adac_encode_1p.inl): every segment must fit sixteen 16-byte chunks per thread of a 1024-thread
// workgroup, counted from the 16-byte boundary at or before its first element
constexpr uint64_t kEncodeOnePassBytes = 16ull * 1024 * 16;
// 64-bit words of device scratch the single-pass encode needs for nseg segments (look-back words, ticket, cursor)
inline uint64_t encode_1p_state_words(uint64_t nseg) { return nseg + 2; }
hipError_t read_encode_stamps(void *host, uint64_t bytes);
// Grouped scans (adac_group_*.inl): all columns belong to one table, `work` and `state` to the first one's layout, keys
// >= ngroups land in bin ngroups, d_validity (may be null) selects rows in the first column's element space.
uint64_t group_sum_partial_bytes();
uint32_t group_sum_max_groups();
uint64_t group_sum_handover_word(uint32_t call_parity); // index (in 64-bit words of the partial buffer) of a call's hand-over word
// SUM(v), COUNT(*) GROUP BY k into d_sums / d_counts, ngroups + 1 words each
hipError_t launch_group_sum(hipStream_t s, const Column &v, const Column &k, const ScanWork &work, uint32_t ngroups,
                            const GroupScanState &state, const uint64_t *d_validity, uint64_t *d_sums, uint64_t *d_counts);
// SUM(a * b) GROUP BY k; d_counts may be null
hipError_t launch_group_product(hipStream_t s, const Column &a, const Column &b, const Column &k, const ScanWork &work,
                                uint32_t ngroups, const GroupScanState &state, const uint64_t *d_validity, uint64_t *d_sums,
                                uint64_t *d_counts);
// SUM(a * b * c) GROUP BY k; d_counts may be null
hipError_t launch_group_product3(hipStream_t s, const Column &a, const Column &b, const Column &c, const Column &k,
                                 const ScanWork &work, uint32_t ngroups, const GroupScanState &state,
                                 const uint64_t *d_validity, uint64_t *d_sums, uint64_t *d_counts);
// COUNT and the six sums of Q1 GROUP BY key in one scan; cols: a, b, c, q, keys; d_out: 7 x (ngroups + 1) words, term t of
// group g at [t * (ngroups + 1) + g]
hipError_t launch_group_q1(hipStream_t s, const Column (&cols)[5], const ScanWork &work, uint32_t ngroups,
                           const GroupScanState &state, const uint64_t *d_validity, uint64_t *d_out);
// Per-segment scans over the scan groups of the first column's layout (`work`); d_validity as above; the caller has
// cleared every output.
// SUM(a * b) into d_sums (adac_sum_product.inl)
hipError_t launch_scan_sum_product(hipStream_t s, const Column &a, const Column &b, const ScanWork &work,
                                   const uint64_t *d_validity, uint64_t *d_sums);
// rows where value(a) <cmp> value(b), cmp an OR of ADAC_CMP_*: d_counts and, unless null, their d_bitmap in a's element
// space (adac_scan_compare.inl)
hipError_t launch_scan_compare(hipStream_t s, const Column &a, const Column &b, const ScanWork &work,
                               const uint64_t *d_validity, uint32_t cmp, uint64_t *d_bitmap, uint64_t *d_counts);
// rows whose value is a member of the bit set d_set over `dom`: d_counts and, unless null, their d_bitmap; and the set built
// from the wanted rows of a column, with the rows inside the domain in d_counts (adac_scan_member.inl)
hipError_t launch_scan_member(hipStream_t s, const Column &col, const ScanWork &work, const uint64_t *d_validity,
                              const uint64_t *d_set, const KeyDomain &dom, uint64_t *d_bitmap, uint64_t *d_counts);
hipError_t launch_scan_member_build(hipStream_t s, const Column &col, const ScanWork &work, const uint64_t *d_validity,
                                    const KeyDomain &dom, uint64_t *d_set, uint64_t *d_counts);
// SUM(value), COUNT(*) GROUP BY key over scan.dom: d_sums (null: no value column is read, `values` is not looked at) and
// d_counts (may be null with d_sums), dom.span words each (adac_group_dense.inl)
hipError_t launch_group_dense(hipStream_t s, const DenseScan &scan, const Column &values, uint64_t *d_sums,
                              uint64_t *d_counts);
// SUM(value), COUNT(*) GROUP BY d_map[key - key_base]: d_sums (null: no value column is read) and d_counts (may be null
// with d_sums), ngroups + 1 words each, entry [ngroups] for the codes >= ngroups (adac_group_mapped.inl)
hipError_t launch_group_mapped(hipStream_t s, const MappedScan &scan, const Column &values, uint64_t *d_sums,
                               uint64_t *d_counts);
// SUM(a * b), SUM(a), COUNT(*) GROUP BY d_map[key - key_base]: d_sums_ab, d_sums_a (may be null) and d_counts (may be
// null), ngroups + 1 words each (adac_group_mapped_product.inl)
hipError_t launch_group_mapped_product(hipStream_t s, const MappedScan &scan, const Column &a, const Column &b,
                                       uint64_t *d_sums_ab, uint64_t *d_sums_a, uint64_t *d_counts);
// d_map[key - key_base] = min(code, 255) for every wanted row inside the domain; the caller has filled d_map
hipError_t launch_build_map(hipStream_t s, const DenseScan &scan, const Column &codes, uint8_t *d_map);
hipError_t launch_encode_1p(hipStream_t s, uint32_t type_size, bool sign_extend, uint64_t null_bits, int rule,
                            int pad_to_byte, adac_segment_desc *d_descs, uint64_t nseg, const void *d_vals,
                            const uint64_t *d_validity, uint64_t *d_minmax, void *d_scan_state, uint64_t *d_words);
hipError_t launch_analyze_packed_g(hipStream_t s, uint32_t type_size, bool sign_extend, uint64_t null_bits, int rule,
                                   const ScanGroup *d_src_groups, uint64_t ngroups, const uint64_t *d_src_words,
                                   const uint64_t *d_validity, uint64_t *d_minmax);
hipError_t launch_repack_g(hipStream_t s, uint32_t type_size, uint64_t null_bits, const ScanGroup *d_src_groups,
                           uint64_t ngroups, const adac_segment_desc *d_dst_descs, const uint64_t *d_src_words,
                           const uint64_t *d_validity, uint64_t *d_dst_words);
// The fused scans' work items as the launchers see them: every group, and the indices of those at widths 2 and 3,
// which a kernel of their own scans (n_narrow is read back once per expansion).
struct ScanGroupList {
	const ScanGroup *d_groups;
	uint64_t ngroups;
	const uint32_t *d_narrow_idx;
	uint32_t n_narrow;
	// arrival cells (see ScanGroupRef), zero between calls; nullptr: the clearing pass + atomics form
	unsigned long long *d_res_cells; // per segment: four words (arrive_sum / arrive_count)
	uint32_t *d_edge_cells;          // two per group: one 64-bit word each (arrive_or)
};
constexpr uint64_t kResCellWords = 4;  // unsigned long long per segment
constexpr uint64_t kEdgeCellWords = 4; // uint32_t per group
hipError_t launch_expand_tiles(hipStream_t s, uint32_t type_size, const adac_segment_desc *d_descs, const TileRef *d_tiles,
                               uint64_t ntiles, TileRec *d_recs);
hipError_t launch_expand_groups(hipStream_t s, const adac_segment_desc *d_descs, const ScanGroupRef *d_refs,
                                uint64_t ngroups, ScanGroup *d_groups, uint32_t *d_narrow_idx, uint32_t *d_narrow_count);
// scan with selection: the rows of the column whose bit is set in d_bitmap to d_out, their element indices to
// d_out_ids unless null, *d_total = rows written.  d_tile_cnt / d_tile_off: ntiles entries of scratch, d_block_tot:
// ceil(ntiles / 1024) words
hipError_t launch_gather_selected(hipStream_t s, const Column &col, const TileRef *d_tiles, uint64_t ntiles,
                                  const TileRec *d_recs, const uint64_t *d_bitmap, uint64_t bitmap_words,
                                  uint32_t *d_tile_cnt, uint64_t *d_tile_off, uint64_t *d_block_tot, void *d_out,
                                  uint64_t *d_out_ids, uint64_t *d_total);
// The fused scans of one column over its layout's groups `gl` (k_scan_agg; col.d_descs plays no part, the groups carry
// the descriptors).  SUM per segment into d_sums
hipError_t launch_scan_sum(hipStream_t s, const Column &col, const ScanGroupList &gl, const uint64_t *d_validity,
                           uint64_t *d_sums);
uint64_t sel_edge_bytes(uint64_t ngroups);
hipError_t launch_sel_merge_edges(hipStream_t s, const void *d_edges, uint64_t ngroups, uint64_t *d_bitmap,
                                  uint64_t tail_word);
// rows with blo <= bits ^ sign bit <= blo + bspan per segment into d_counts and, unless null, their d_bitmap; the words
// of the bitmap that groups share go to d_edges (launch_sel_merge_edges stores them) or through the edge cells
hipError_t launch_scan_count_range(hipStream_t s, const Column &col, const ScanGroupList &gl, const uint64_t *d_validity,
                                   uint64_t blo, uint64_t bspan, uint64_t *d_counts, uint64_t *d_bitmap, void *d_edges,
                                   bool edge_cells, uint64_t tail_word);

// Persistent block images (adac_block_image.inl): one segment's packed words <-> its image in a block buffer.
struct BlockJob {
	uint64_t word_off;   // first word of the segment in the packed arena
	uint64_t block_off;  // byte offset of its image in the block buffer, multiple of 8
	uint64_t min;
	uint64_t bit_size;   // count * width: the int_vector's m_size
	uint32_t nwords;     // ceil(bit_size / 64)
	uint32_t arena_words; // words the segment owns in the arena (parse: the tail past nwords is zeroed)
	uint8_t width, flags, type, pad[5];
};
static_assert(sizeof(BlockJob) == 48, "device record");
hipError_t launch_blocks_write(hipStream_t s, const BlockJob *d_jobs, uint64_t njobs, uint32_t max_units,
                               const uint64_t *d_words, void *d_blocks);
hipError_t launch_blocks_read(hipStream_t s, const BlockJob *d_jobs, uint64_t njobs, uint32_t max_units,
                              const void *d_blocks, uint64_t *d_words, uint32_t *d_bad);

// DuckDB BITPACKING segments (adac_bitpacking.inl).  Host view of one metadata group; must match BpGroup.
struct BpGroupHost {
	uint64_t block_off;
	uint64_t out_off;
	uint32_t group;
	uint32_t rows;
	uint64_t payload_off, frame, extra; // parsed header, filled on the device by launch_bp_prepare
	uint32_t mode, width;
};
// compress side: per-group statistics (device -> host) and write records (host -> device); must match
// BpStats / BpWrite in adac_bitpacking.inl
struct BpStatsHost {
	uint64_t bmin, bmax, bdmin, bdmax, v0;
	uint32_t rows, nvalid, delta_overflow, pad;
};
struct BpWriteHost {
	uint64_t frame, extra, first;
	uint32_t seg, data_off, meta_off, mode, width, rows, first_of_segment, pad;
};
hipError_t launch_bp_stats(hipStream_t s, uint32_t type_size, bool is_signed, const void *d_vals,
                           const uint64_t *d_validity, uint64_t n, void *d_stats);
hipError_t launch_bp_write(hipStream_t s, uint32_t type_size, const void *d_recs, uint64_t ngroups, const void *d_vals,
                           const uint64_t *d_validity, uint64_t block_stride, void *d_blocks);
hipError_t launch_bp_prepare(hipStream_t s, uint32_t type_size, void *d_groups, uint64_t ngroups, const void *d_blocks);
// A BITPACKING column: its type, its parsed group table (launch_bp_prepare's) and the blocks buffer it is bound to.
struct BpColumn {
	const void *d_groups, *d_blocks;
	uint32_t type_size;
	bool is_signed;
};
// decode: every group, or `count` rows from row skip_first of group group0 to d_out + out_off
hipError_t launch_bp_unpack(hipStream_t s, const BpColumn &col, uint64_t ngroups, void *d_out);
hipError_t launch_bp_unpack_range(hipStream_t s, const BpColumn &col, uint32_t group0, uint32_t skip_first, uint64_t count,
                                  uint64_t out_off, void *d_out);
hipError_t launch_bp_fetch(hipStream_t s, uint32_t type_size, const uint64_t *d_block_offs, const void *d_blocks,
                           const uint32_t *d_segs, const uint32_t *d_rows, uint64_t n, void *d_out);
// fused scans on the block images (adac_bp_scans.inl); op values match kBpScanSum / Range / MinMax there.  d_res:
// sums | counts | min, max pairs per segment (d_group_seg: the segment of every group); the caller has filled it (and
// the bitmap) - see the kernel's header
enum : int { kBpScanOpSum = 0, kBpScanOpRange = 1, kBpScanOpMinMax = 2 };
hipError_t launch_bp_scan(hipStream_t s, const BpColumn &col, int op, const uint32_t *d_group_seg, uint64_t ngroups,
                          const uint64_t *d_validity, uint64_t blo, uint64_t bspan, uint64_t *d_res, uint64_t *d_bitmap);
hipError_t launch_bp_scan_minmax_finish(hipStream_t s, uint32_t type_size, bool is_signed, uint64_t *d_minmax,
                                        uint64_t nseg);
// pair scans on the block images of two layouts whose group tables agree (adac_bp_pair_scans.inl).  The caller has
// zeroed the results.  SUM(a * b) per segment of a (d_group_seg: a's)
hipError_t launch_bp_scan_pair_sum(hipStream_t s, const BpColumn &a, const BpColumn &b, const uint32_t *d_group_seg,
                                   uint64_t ngroups, const uint64_t *d_validity, uint64_t *d_sums);
// SUM(v), COUNT(*) GROUP BY k, keys >= nkeys in bin nkeys; d_counts may be null
hipError_t launch_bp_scan_pair_gsum(hipStream_t s, const BpColumn &v, const BpColumn &k, uint64_t ngroups,
                                    const uint64_t *d_validity, uint32_t nkeys, uint64_t *d_sums, uint64_t *d_counts);
// rows where value(a) <cmp> value(b), cmp an OR of ADAC_CMP_*: d_counts per segment of a and, unless nullptr, d_bitmap
// in a's element space
hipError_t launch_bp_scan_pair_cmp(hipStream_t s, const BpColumn &a, const BpColumn &b, const uint32_t *d_group_seg,
                                   uint64_t ngroups, const uint64_t *d_validity, uint32_t cmp, uint64_t *d_counts,
                                   uint64_t *d_bitmap);
// scan with selection on the block images (adac_bp_select_gather.inl): the rows whose bit is set in d_bitmap to d_out,
// their element indices to d_out_ids unless null, *d_total = rows written.  d_group_cnt / d_group_off: ngroups entries
// of scratch, d_block_tot: ceil(ngroups / 1024) words
hipError_t launch_bp_gather_selected(hipStream_t s, const BpColumn &col, uint64_t ngroups, const uint64_t *d_bitmap,
                                     uint32_t *d_group_cnt, uint64_t *d_group_off, uint64_t *d_block_tot, void *d_out,
                                     uint64_t *d_out_ids, uint64_t *d_total);

} // namespace adac
