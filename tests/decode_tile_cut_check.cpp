// Stand-alone check of the decode's tile cut (csrc/adac_tile_cut.h), built with -fsanitize=address,undefined and run by
// tests/test_decode_tile_cut_host.py.  No device code, nothing loaded into Python.
//
//   decode_tile_cut_check                               built-in segment lists at every type size
//   decode_tile_cut_check TYPE_SIZE COUNTS.bin [OFFS.bin]   uint32 counts (uint64 element offsets) from files; prints
//                                                       "tiles N static_rows R rows T"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "adac_tile_cut.h"

using adac::TileRef;

#define CHECK(cond, ...)                                                                                               \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			std::fprintf(stderr, "FAILED %s (line %d): ", #cond, __LINE__);                                            \
			std::fprintf(stderr, __VA_ARGS__);                                                                         \
			std::fprintf(stderr, "\n");                                                                                \
			std::exit(1);                                                                                              \
		}                                                                                                              \
	} while (0)

struct Stats {
	uint64_t tiles = 0, static_rows = 0, rows = 0;
};

// every invariant of the cut over one segment list; offs == nullptr: back to back from element 0
static Stats check_list(uint32_t ts, const std::vector<uint32_t> &counts, const uint64_t *offs) {
	const uint32_t TILE = adac::kCutTileBytes / ts, L = adac::kCutLineBytes / ts, K = 16 / ts;
	const std::vector<TileRef> tiles = adac::cut_tiles_on_lines(ts, counts.data(), offs, counts.size());
	Stats st;
	st.tiles = tiles.size();
	size_t t = 0;
	uint64_t run = 0;
	for (size_t s = 0; s < counts.size(); s++) {
		const uint64_t off = offs ? offs[s] : run;
		run = off + counts[s];
		st.rows += counts[s];
		uint32_t next = 0; // the tiles of a segment are in order and partition it
		bool head = true;
		while (next < counts[s]) {
			CHECK(t < tiles.size(), "segment %zu: rows from %u have no tile", s, next);
			const TileRef r = tiles[t++];
			CHECK(r.seg == s, "tile %zu belongs to segment %u, expected %zu", t - 1, r.seg, s);
			CHECK(r.first == next, "segment %zu: tile at row %u, expected %u", s, r.first, next);
			const uint32_t n = adac::cut_tile_rows(ts, counts[s], off, r.first);
			CHECK(n >= 1 && n <= TILE, "segment %zu row %u: %u rows", s, r.first, n);
			CHECK(n <= counts[s] - r.first, "segment %zu row %u: %u rows run past the segment", s, r.first, n);
			if (!head) CHECK(((off + r.first) & (L - 1)) == 0, "segment %zu: tile at row %u starts off a line", s, r.first);
			// all but the head and the last are full; a segment on a line is cut exactly as the segment-relative table
			if (!head && r.first + n < counts[s]) CHECK(n == TILE, "segment %zu row %u: inner tile of %u rows", s, r.first, n);
			if ((off & (L - 1)) == 0) {
				CHECK(r.first % TILE == 0, "segment %zu on a line: tile at row %u", s, r.first);
				const uint32_t left = counts[s] - r.first;
				CHECK(n == (left < TILE ? left : TILE), "segment %zu on a line: %u rows at row %u", s, n, r.first);
			}
			if (n == TILE && ((off + r.first) & (K - 1)) == 0) st.static_rows += n; // decode_tile's fast-path test
			next += n;
			head = false;
		}
		CHECK(next == counts[s], "segment %zu: tiles cover %u of %u rows", s, next, counts[s]);
	}
	CHECK(t == tiles.size(), "%zu tiles belong to no segment", tiles.size() - t);
	return st;
}

static std::vector<uint64_t> read_file(const char *path, size_t elem) {
	FILE *f = std::fopen(path, "rb");
	CHECK(f != nullptr, "cannot open %s", path);
	std::fseek(f, 0, SEEK_END);
	const long bytes = std::ftell(f);
	std::fseek(f, 0, SEEK_SET);
	CHECK(bytes >= 0 && (size_t)bytes % elem == 0, "%s: %ld bytes", path, bytes);
	std::vector<unsigned char> raw((size_t)bytes);
	if (bytes) CHECK(std::fread(raw.data(), 1, raw.size(), f) == raw.size(), "short read of %s", path);
	std::fclose(f);
	std::vector<uint64_t> out(raw.size() / elem);
	for (size_t i = 0; i < out.size(); i++) {
		uint64_t v = 0;
		for (size_t b = 0; b < elem; b++) v |= (uint64_t)raw[i * elem + b] << (8 * b);
		out[i] = v;
	}
	return out;
}

static void builtin() {
	for (uint32_t ts : {1u, 2u, 4u, 8u}) {
		const uint32_t TILE = adac::kCutTileBytes / ts, L = adac::kCutLineBytes / ts, K = 16 / ts;
		// no segments: no tiles, with and without a counts pointer
		CHECK(adac::cut_tiles_on_lines(ts, nullptr, nullptr, 0).empty(), "nseg == 0 yields tiles");
		CHECK(check_list(ts, {}, nullptr).tiles == 0, "empty list yields tiles");
		CHECK(check_list(ts, {0, 0, 0}, nullptr).tiles == 0, "empty segments yield tiles");
		const uint32_t sizes[] = {1, K - 1 ? K - 1 : 1, L - 1, L, TILE - L, TILE - 1, TILE, TILE + 1, TILE + L - 1, 2 * TILE,
		                          2 * TILE + 1};
		// every size at every start phase that matters, as a gapped list: one segment per (phase, size)
		const uint32_t phases[] = {0, 1, K - 1, K, K + 1, L - 1};
		std::vector<uint32_t> counts;
		std::vector<uint64_t> offs;
		uint64_t at = 0;
		for (uint32_t ph : phases) {
			for (uint32_t n : sizes) {
				at = (at + L - 1) / L * L + ph;
				offs.push_back(at);
				counts.push_back(n);
				at += n;
			}
		}
		const Stats g = check_list(ts, counts, offs.data());
		CHECK(g.rows > 0 && g.tiles >= counts.size(), "gapped list: %llu tiles", (unsigned long long)g.tiles);
		// the same sizes back to back (the phases then follow from the running sum), an empty segment in the middle
		std::vector<uint32_t> dense(sizes, sizes + sizeof(sizes) / sizeof(sizes[0]));
		dense.insert(dense.begin() + 4, 0u);
		dense.insert(dense.begin(), 3u);
		check_list(ts, dense, nullptr);
		// a head tile: TILE - ph rows, then whole tiles from a line
		const uint64_t off1[] = {L + 1};
		const std::vector<TileRef> h = adac::cut_tiles_on_lines(ts, std::vector<uint32_t> {3 * TILE}.data(), off1, 1);
		CHECK(h.size() == 4 && h[1].first == TILE - 1 && h[2].first == 2 * TILE - 1 && h[3].first == 3 * TILE - 1,
		      "head tile of a segment one element past a line");
		// element offsets beyond 2^32 and a count at the type's limit of the table (uint32 rows)
		const uint64_t off2[] = {(1ull << 40) + L - 1};
		check_list(ts, {0xffffffffu / 64}, off2);
	}
}

int main(int argc, char **argv) {
	if (argc == 1) {
		builtin();
		std::printf("ok\n");
		return 0;
	}
	CHECK(argc == 3 || argc == 4, "usage: %s [TYPE_SIZE COUNTS.bin [OFFS.bin]]", argv[0]);
	const uint32_t ts = (uint32_t)std::atoi(argv[1]);
	CHECK(ts == 1 || ts == 2 || ts == 4 || ts == 8, "type size %u", ts);
	const std::vector<uint64_t> c64 = read_file(argv[2], 4);
	std::vector<uint32_t> counts(c64.begin(), c64.end());
	std::vector<uint64_t> offs;
	if (argc == 4) {
		offs = read_file(argv[3], 8);
		CHECK(offs.size() == counts.size(), "%zu offsets for %zu counts", offs.size(), counts.size());
	}
	const Stats st = check_list(ts, counts, argc == 4 ? offs.data() : nullptr);
	std::printf("tiles %llu static_rows %llu rows %llu\n", (unsigned long long)st.tiles,
	            (unsigned long long)st.static_rows, (unsigned long long)st.rows);
	return 0;
}
