// adac_tile_cut.h — the decode's tile table: segments cut on 128-byte lines of the OUTPUT.  Pure host code, no HIP: the
// layout (adac_capi.cpp) builds the table with it and tests/test_decode_tile_cut_host.py checks it stand-alone.
#pragma once

#include <stdint.h>

#include <vector>

namespace adac {

constexpr uint32_t kCutTileBytes = 16384; // == kTileBytes (adac_internal.h asserts it)
constexpr uint32_t kCutLineBytes = 128;   // one output cache line

// One tile of one segment: rows [first, first + n) with n a function of the segment and `first` alone (cut_tile_rows
// for the decode's table, min(count - first, TILE) for the segment-relative one).
struct TileRef {
	uint32_t seg;
	uint32_t first;
};

// Rows of the tile that starts at row `first` of a segment whose row 0 is element `val_off` of the output: up to the end
// of the segment, and never past the TILE rows that begin at the line holding the tile's first element.  A tile that
// starts on a line is a whole TILE (or the segment's rest); one that starts `ph` elements past a line has TILE - ph rows,
// so the next one starts on a line.  k_unpack computes the same expression (unpack_tile_rows).
inline uint32_t cut_tile_rows(uint32_t type_size, uint32_t count, uint64_t val_off, uint32_t first) {
	const uint32_t tile = kCutTileBytes / type_size;
	const uint32_t line = kCutLineBytes / type_size;
	const uint32_t room = tile - (uint32_t)((val_off + first) & (line - 1));
	const uint32_t left = count - first;
	return left < room ? left : room;
}

// The decode's tiles of `nseg` segments, in segment order: a segment that starts off a line gets a short head tile, every
// later tile starts on a line, and all but a segment's last are full.  val_offs == nullptr: the segments lie back to back
// from element 0.  Segments that start on a line are cut exactly as the segment-relative table cuts them.
inline std::vector<TileRef> cut_tiles_on_lines(uint32_t type_size, const uint32_t *counts, const uint64_t *val_offs,
                                               uint64_t nseg) {
	std::vector<TileRef> tiles;
	uint64_t run = 0;
	for (uint64_t s = 0; s < nseg; s++) {
		const uint64_t off = val_offs ? val_offs[s] : run;
		run = off + counts[s];
		for (uint32_t first = 0; first < counts[s]; first += cut_tile_rows(type_size, counts[s], off, first)) {
			tiles.push_back(TileRef {(uint32_t)s, first});
		}
	}
	return tiles;
}

} // namespace adac
