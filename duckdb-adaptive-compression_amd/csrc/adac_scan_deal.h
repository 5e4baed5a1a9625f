// adac_scan_deal.h — the fused scans' work items: a segment's tiles dealt evenly to scan groups, and the arrival cells
// of the bitmap words that groups share.  Pure host code, no HIP: the layout (adac_capi.cpp) builds its group table with
// it and tests/test_owned_groups_host.py checks it stand-alone.
#pragma once

#include <stdint.h>

#include <vector>

namespace adac {

constexpr uint32_t kDealTileBytes = 16384;      // == kTileBytes (adac_internal.h asserts it)
constexpr uint32_t kDealMaxGroupRows = 65536;   // the selection scan's LDS image holds 64 Ki rows

// Work item of the fused scans before its segment's descriptor is folded in (ScanGroup, adac_internal.h): rows
// [first, first + rows) of ONE segment, static per layout and grouping.
// The ARRIVAL fields (round 3) let a scan finish its results inside the one kernel — no clearing pass before it and no
// merge kernel after it: `seg_groups` groups add into the segment's result cell and the last one to arrive stores the
// total; a bitmap word that several groups cover in part (dense value spaces only) is ORed into an edge cell by
// `n_first` / `n_last` groups and stored by the last of them.  Cells are zero between calls (the last arriver resets).
struct ScanGroupRef {
	uint32_t seg;
	uint32_t first;
	uint32_t rows; // a segment's tiles are dealt evenly to its groups, so group sizes differ between segments
	uint32_t seg_groups; // scan groups of this segment
	uint32_t cell_first; // edge cell of the group's first bitmap word when that word is covered in part
	uint32_t cell_last;  // ... of its last word (groups of more than one word)
	uint16_t n_first;    // groups that cover the first word in part (0: the word is whole, or the value space has gaps)
	uint16_t n_last;
	uint32_t pad;
};
static_assert(sizeof(ScanGroupRef) == 32, "device record");

// Tiles per scan group.  A segment's tiles are dealt EVENLY to ceil(tiles / target) workgroups.  Default target
// (knob < 1): 12 tiles of u64, 6 of u32 (~24 K rows), 8 of u16, 4 of u8 (64 K rows): a 16-tile DuckDB segment becomes
// two to four groups.  Measured (tools/ab_tuning.py, 400 M rows): a whole 32 767-row segment per workgroup puts the
// workgroups' packed streams and bitmap regions at the same power-of-two stride (32 KiB / 4 KiB) and costs 6-25 %;
// 16-24 K rows is the best of 4 .. 32 tiles (u8 and u16 want more rows per workgroup).
inline int scan_tiles_per_group(uint32_t type_size, int knob) {
	const uint32_t tile = kDealTileBytes / type_size;
	int per = knob;
	if (per < 1) per = type_size == 8 ? 12 : type_size == 4 ? 6 : type_size == 2 ? 8 : 4;
	if ((uint64_t)per * tile > kDealMaxGroupRows) per = (int)(kDealMaxGroupRows / tile);
	return per;
}

// The scan groups of `nseg` segments at `per` tiles per group, in segment order (a segment without rows has none).
// dense_values (the segments lie back to back from element 0): the arrival cells of shared bitmap words are assigned.
inline std::vector<ScanGroupRef> deal_scan_groups(uint32_t type_size, const uint32_t *counts, const uint64_t *val_offs,
                                                  uint64_t nseg, bool dense_values, int per) {
	const uint32_t tile = kDealTileBytes / type_size;
	std::vector<ScanGroupRef> refs;
	for (uint64_t s = 0; s < nseg; s++) {
		const uint64_t ntiles = ((uint64_t)counts[s] + tile - 1) / tile;
		if (ntiles == 0) continue;
		const uint64_t ngroups = (ntiles + (uint64_t)per - 1) / (uint64_t)per;
		const uint64_t rows_per_group = ((ntiles + ngroups - 1) / ngroups) * tile;
		const size_t seg_first = refs.size();
		for (uint64_t first = 0; first < counts[s]; first += rows_per_group) {
			const uint64_t left = counts[s] - first;
			ScanGroupRef r {};
			r.seg = (uint32_t)s;
			r.first = (uint32_t)first;
			r.rows = (uint32_t)(left < rows_per_group ? left : rows_per_group);
			refs.push_back(r);
		}
		for (size_t g = seg_first; g < refs.size(); g++) refs[g].seg_groups = (uint32_t)(refs.size() - seg_first);
	}
	if (!dense_values) return refs;
	// Bitmap words that groups cover in part (sel_write_out's test: word 0 of a group unless the group starts on a
	// word boundary and fills it; its last word, if it has more than one, unless it ends on a boundary).  The
	// groups are in element order, so the arrivals at one word are neighbours in this list: a run of equal words
	// shares the cell named after its first arrival and expects as many arrivals as the run is long.
	struct Arrival {
		uint64_t word;
		uint32_t group, which;
	};
	std::vector<Arrival> arr;
	for (size_t g = 0; g < refs.size(); g++) {
		const uint64_t p0 = val_offs[refs[g].seg] + refs[g].first, p1 = p0 + refs[g].rows;
		const uint64_t nwords = ((p1 + 31) >> 5) - (p0 >> 5);
		if (!((p0 & 31) == 0 && p0 + 32 <= p1)) arr.push_back(Arrival {p0 >> 5, (uint32_t)g, 0u});
		if (nwords > 1 && (p1 & 31) != 0) arr.push_back(Arrival {(p1 - 1) >> 5, (uint32_t)g, 1u});
	}
	for (size_t a = 0; a < arr.size();) {
		size_t b = a;
		while (b < arr.size() && arr[b].word == arr[a].word) b++;
		const uint32_t cell = 2u * arr[a].group + arr[a].which;
		const uint16_t n = (uint16_t)(b - a); // a word holds 32 rows and every group at least one: n <= 32
		for (size_t i = a; i < b; i++) {
			ScanGroupRef &r = refs[arr[i].group];
			if (arr[i].which == 0) {
				r.cell_first = cell;
				r.n_first = n;
			} else {
				r.cell_last = cell;
				r.n_last = n;
			}
		}
		a = b;
	}
	return refs;
}

} // namespace adac
