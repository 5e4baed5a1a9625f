// Stand-alone check of the buffer owner (csrc/adac_owned.h) and of the scan-group deal (csrc/adac_scan_deal.h), built
// with -fsanitize=address,undefined and run by tests/test_owned_groups_host.py.  No device code, nothing loaded into
// Python.  The owner's memory calls are defined HERE: malloc / free behind a counter that refuses the k-th allocation,
// so a leak, a double free or a use after free on a failure path is the sanitizer's to report.
//
//   owned_groups_check                 every check below
//   owned_groups_check per TYPE_SIZE   prints the default tiles per scan group of that type size
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "adac_owned.h"
#include "adac_scan_deal.h"

using adac::DeviceArray;
using adac::Mem;
using adac::Owned;
using adac::ScanGroupRef;

#define CHECK(cond, ...)                                                                                               \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			std::fprintf(stderr, "FAILED %s (line %d): ", #cond, __LINE__);                                            \
			std::fprintf(stderr, __VA_ARGS__);                                                                         \
			std::fprintf(stderr, "\n");                                                                                \
			std::exit(1);                                                                                              \
		}                                                                                                              \
	} while (0)

// ---- the counting allocator ----------------------------------------------------------------------------------------
static int g_allocs = 0, g_frees = 0, g_live = 0;
static int g_fail_at = 0; // the allocation with this number (1-based, since the last arm()) fails; 0 = none
static size_t g_last_bytes = 0;
constexpr int kOutOfMemory = 2;

static void arm(int fail_at) { g_allocs = g_frees = 0, g_fail_at = fail_at; }

int adac::owned_alloc(Mem kind, void **p, size_t bytes) {
	if (++g_allocs == g_fail_at) return kOutOfMemory;
	CHECK((kind == Mem::Event) == (bytes == 0), "%zu bytes asked for kind %d", bytes, (int)kind);
	g_last_bytes = bytes;
	*p = std::malloc(bytes ? bytes : 1); // exactly the bytes asked for: one past them is the sanitizer's to catch
	CHECK(*p != nullptr, "malloc");
	g_live++;
	return 0;
}
int adac::owned_free(Mem, void *p) {
	CHECK(p != nullptr, "null pointer freed");
	std::free(p);
	g_frees++, g_live--;
	return 0;
}

struct OpaqueEvent; // stands for the runtime's event struct: never complete
using Event = Owned<OpaqueEvent, Mem::Event>;
using PinnedWord = Owned<uint32_t, Mem::Pinned>;

// ---- one owner -----------------------------------------------------------------------------------------------------
static void check_owner() {
	arm(0);
	{
		DeviceArray<uint64_t> a;
		CHECK(!a && a.get() == nullptr && a.size() == 0, "a fresh owner is not empty");
		a.reset(); // no-op on an empty owner
		CHECK(g_frees == 0 && g_allocs == 0, "reset() of an empty owner called the allocator");
		// n == 0: one element, not null
		CHECK(a.alloc(0) == 0 && a.get() != nullptr && a.size() == 0, "alloc(0)");
		CHECK(g_last_bytes == sizeof(uint64_t) && a.bytes() == sizeof(uint64_t), "alloc(0): %zu bytes", g_last_bytes);
		a[0] = 7;
		CHECK(a.alloc(5) == 0 && a.size() == 5 && g_last_bytes == 5 * sizeof(uint64_t) && g_frees == 1, "alloc(5) over alloc(0)");
		for (int i = 0; i < 5; i++) a[i] = i;
		uint64_t *const pa = a.get();
		// move construction: the source is empty, nothing is freed
		DeviceArray<uint64_t> b(std::move(a));
		CHECK(!a && a.size() == 0 && b.get() == pa && b.size() == 5 && g_frees == 1, "move construction");
		// move assignment: the destination's old buffer is freed exactly once, the source is empty
		DeviceArray<uint64_t> c;
		CHECK(c.alloc(3) == 0, "alloc(3)");
		c = std::move(b);
		CHECK(!b && b.size() == 0 && c.get() == pa && c.size() == 5 && g_frees == 2 && g_live == 1, "move assignment");
		CHECK(c[4] == 4, "the moved buffer lost its contents");
		c = std::move(b); // from an empty owner: c is emptied, its buffer freed once
		CHECK(!c && g_frees == 3 && g_live == 0, "move assignment from an empty owner");
		c.reset();
		CHECK(g_frees == 3, "reset() freed twice");
		// a failed alloc() leaves the current buffer where it is
		CHECK(c.alloc(2) == 0, "alloc(2)");
		c[1] = 11;
		uint64_t *const pc = c.get();
		arm(1);
		CHECK(c.alloc(9) == kOutOfMemory && c.get() == pc && c.size() == 2 && c[1] == 11 && g_frees == 0, "failed alloc()");
		arm(0);
		Event ev;
		PinnedWord w;
		CHECK(ev.alloc(1) == 0 && ev.get() != nullptr && w.alloc(1) == 0, "event / pinned word");
		*w = 0;
	}
	CHECK(g_live == 0, "%d buffers outlive their owners", g_live);
}

// ---- groups --------------------------------------------------------------------------------------------------------
// The layout's four tables of one deal; the narrow-count trio (device word, pinned word, event); the gather's scratch.
struct Tables {
	DeviceArray<ScanGroupRef> refs;
	DeviceArray<uint64_t> groups;
	DeviceArray<uint32_t> narrow_idx, edge_cells;
	int alloc(size_t n) { return adac::alloc_group(refs, n, groups, n, narrow_idx, n, edge_cells, 4 * n); }
	bool none() const { return !refs && !groups && !narrow_idx && !edge_cells; }
	bool all() const { return refs && groups && narrow_idx && edge_cells; }
};
struct Trio {
	DeviceArray<uint32_t> d_count;
	PinnedWord h_count;
	Event ev;
	int alloc() { return adac::alloc_group(d_count, 1, h_count, 1, ev, 1); }
	bool none() const { return !d_count && !h_count && !ev; }
	bool all() const { return d_count && h_count && ev; }
};
struct Scratch {
	DeviceArray<uint32_t> cnt;
	DeviceArray<uint64_t> off, tot;
	int ensure(size_t n) { return adac::ensure_group(cnt, n, off, n, tot, (n + 1023) / 1024 + 1); }
	bool none() const { return !cnt && !off && !tot; }
	bool all() const { return cnt && off && tot; }
};

template <class G, class Alloc>
static void check_group(int members, Alloc alloc) {
	for (int k = 1; k <= members; k++) {
		G g;
		arm(k);
		CHECK(alloc(g) == kOutOfMemory, "allocation %d of %d did not fail", k, members);
		CHECK(g_allocs == k, "%d allocator calls after a failure at call %d", g_allocs, k);
		CHECK(g.none(), "a member is set after a failure at call %d", k);
		CHECK(g_live == 0 && g_frees == k - 1, "failure at call %d: %d buffers live, %d freed", k, g_live, g_frees);
		arm(0); // a second attempt on a healthy allocator
		CHECK(alloc(g) == 0 && g.all() && g_allocs == members && g_live == members, "second attempt after a failure at %d", k);
	}
	CHECK(g_live == 0, "%d buffers outlive their group", g_live);
}

static void check_groups() {
	for (size_t n : {(size_t)0, (size_t)1, (size_t)37}) {
		check_group<Tables>(4, [n](Tables &t) { return t.alloc(n); });
		check_group<Scratch>(3, [n](Scratch &s) { return s.ensure(n); });
	}
	check_group<Trio>(3, [](Trio &t) { return t.alloc(); });
	// a group that is there is left alone
	Scratch s;
	arm(0);
	CHECK(s.ensure(5) == 0 && g_allocs == 3, "ensure");
	uint32_t *const p = s.cnt.get();
	arm(1);
	CHECK(s.ensure(5) == 0 && g_allocs == 0 && s.cnt.get() == p, "ensure_group on a group that is there called the allocator");
	// n == 0: every member one element
	Tables z;
	arm(0);
	CHECK(z.alloc(0) == 0 && z.all() && z.edge_cells.bytes() == sizeof(uint32_t), "group of empty arrays");
	z.refs[0] = ScanGroupRef {};
	z.edge_cells[0] = 0;

	// A re-deal: the new tables are built in locals and moved in only when all is done.  A failure at any allocation
	// leaves the previous tables, untouched; success frees each of them exactly once.
	Tables cur;
	arm(0);
	CHECK(cur.alloc(8) == 0, "first deal");
	for (int i = 0; i < 8; i++) cur.narrow_idx[i] = 100 + i;
	ScanGroupRef *const old_refs = cur.refs.get();
	for (int k = 1; k <= 4; k++) {
		Tables next;
		arm(k);
		CHECK(next.alloc(21) == kOutOfMemory && next.none(), "re-deal: failure at call %d", k);
		CHECK(cur.all() && cur.refs.get() == old_refs && cur.refs.size() == 8 && cur.narrow_idx[7] == 107,
		      "re-deal: a failure at call %d touched the tables in place", k);
	}
	{
		Tables next;
		arm(0);
		CHECK(next.alloc(21) == 0, "re-deal");
		// an enqueue that is refused after the allocation: `next` goes, the layout keeps its tables
	}
	CHECK(g_live == 4 + 3 + 4 && cur.narrow_idx[0] == 100, "an abandoned build left %d buffers", g_live);
	{
		Tables next;
		arm(0);
		CHECK(next.alloc(21) == 0, "re-deal");
		cur = std::move(next); // commit
		CHECK(g_frees == 4 && next.none() && cur.all() && cur.refs.size() == 21, "commit: %d buffers freed", g_frees);
		for (int i = 0; i < 21; i++) cur.narrow_idx[i] = i;
	}
	// alloc_group over members that are set: replaced together or not at all
	arm(3);
	uint32_t *const idx = cur.narrow_idx.get();
	CHECK(cur.alloc(5) == kOutOfMemory && cur.narrow_idx.get() == idx && cur.refs.size() == 21 && cur.narrow_idx[20] == 20,
	      "a failed alloc_group changed members that were set");
	arm(0);
	CHECK(cur.alloc(5) == 0 && cur.refs.size() == 5 && cur.edge_cells.size() == 20 && g_frees == 4, "alloc_group over a set group");
}

// ---- the deal ------------------------------------------------------------------------------------------------------
// Every invariant of the deal over one segment list, against a recount of its own.  Returns the groups per segment.
static std::vector<uint32_t> check_deal(uint32_t ts, const std::vector<uint32_t> &counts, const std::vector<uint64_t> &offs,
                                        bool dense, int per) {
	const uint32_t tile = adac::kDealTileBytes / ts;
	const std::vector<ScanGroupRef> refs = adac::deal_scan_groups(ts, counts.data(), offs.data(), counts.size(), dense, per);
	std::vector<uint32_t> per_seg(counts.size(), 0);
	size_t g = 0;
	for (size_t s = 0; s < counts.size(); s++) {
		uint64_t next = 0; // the groups of a segment are in order and partition its rows
		const size_t g0 = g;
		while (next < counts[s]) {
			CHECK(g < refs.size(), "segment %zu: rows from %llu have no group", s, (unsigned long long)next);
			const ScanGroupRef &r = refs[g++];
			CHECK(r.seg == s && r.first == next, "group %zu: segment %u row %u, expected %zu row %llu", g - 1, r.seg, r.first, s,
			      (unsigned long long)next);
			CHECK(r.rows >= 1 && r.rows <= adac::kDealMaxGroupRows, "group %zu: %u rows", g - 1, r.rows);
			CHECK(r.rows <= (uint64_t)per * tile, "group %zu: %u rows at %d tiles per group", g - 1, r.rows, per);
			CHECK(r.first % tile == 0, "group %zu starts inside a tile (row %u)", g - 1, r.first);
			next += r.rows;
		}
		CHECK(next == counts[s], "segment %zu: groups cover %llu of %u rows", s, (unsigned long long)next, counts[s]);
		per_seg[s] = (uint32_t)(g - g0);
		const uint64_t ntiles = ((uint64_t)counts[s] + tile - 1) / tile;
		CHECK(per_seg[s] <= (ntiles + per - 1) / per, "segment %zu: %u groups for %llu tiles", s, per_seg[s],
		      (unsigned long long)ntiles);
		for (size_t i = g0; i < g; i++) {
			CHECK(refs[i].seg_groups == per_seg[s], "group %zu: seg_groups %u of %u", i, refs[i].seg_groups, per_seg[s]);
		}
	}
	CHECK(g == refs.size(), "%zu groups belong to no segment", refs.size() - g);
	// the 32-row bitmap words a group covers in part, recounted word by word: who arrives where
	struct Arrival {
		size_t group;
		bool last;
	};
	std::map<uint64_t, std::vector<Arrival>> at;
	for (size_t i = 0; i < refs.size(); i++) {
		const uint64_t p0 = offs[refs[i].seg] + refs[i].first, p1 = p0 + refs[i].rows;
		bool first_part = false, last_part = false;
		for (uint64_t w = p0 / 32; w * 32 < p1; w++) {
			const uint64_t lo = w * 32 > p0 ? w * 32 : p0, hi = (w + 1) * 32 < p1 ? (w + 1) * 32 : p1;
			if (hi - lo == 32) continue;
			CHECK(w == p0 / 32 || w == (p1 - 1) / 32, "group %zu covers an inner word in part", i);
			const bool last = w != p0 / 32;
			(last ? last_part : first_part) = true;
			if (dense) at[w].push_back(Arrival {i, last});
		}
		if (!dense || !first_part) CHECK(refs[i].n_first == 0 && refs[i].cell_first == 0, "group %zu: first-word cell", i);
		if (!dense || !last_part) CHECK(refs[i].n_last == 0 && refs[i].cell_last == 0, "group %zu: last-word cell", i);
	}
	std::map<uint32_t, uint64_t> cell_word;
	for (const auto &wa : at) {
		const std::vector<Arrival> &a = wa.second;
		CHECK(a.size() <= 32, "%zu arrivals at one word", a.size());
		const ScanGroupRef &r0 = refs[a[0].group];
		const uint32_t cell = a[0].last ? r0.cell_last : r0.cell_first;
		CHECK(cell < 2 * refs.size(), "cell %u of %zu groups", cell, refs.size());
		CHECK(cell_word.emplace(cell, wa.first).second, "cell %u serves two words", cell);
		for (const Arrival &x : a) {
			const ScanGroupRef &r = refs[x.group];
			CHECK((x.last ? r.cell_last : r.cell_first) == cell, "word %llu: its arrivals use different cells",
			      (unsigned long long)wa.first);
			CHECK((x.last ? r.n_last : r.n_first) == a.size(), "word %llu: group %zu expects %u arrivals of %zu",
			      (unsigned long long)wa.first, x.group, x.last ? r.n_last : r.n_first, a.size());
		}
	}
	return per_seg;
}

static std::vector<uint64_t> back_to_back(const std::vector<uint32_t> &counts) {
	std::vector<uint64_t> offs;
	uint64_t run = 0;
	for (uint32_t c : counts) {
		offs.push_back(run);
		run += c;
	}
	return offs;
}

static void check_deals() {
	const int defaults[] = {0, 4, 8, 0, 6, 0, 0, 0, 12}; // by type size: 6 x 4096 rows at 4 bytes, 12 x 2048 at 8
	for (uint32_t ts : {1u, 2u, 4u, 8u}) {
		const uint32_t tile = adac::kDealTileBytes / ts;
		CHECK(adac::scan_tiles_per_group(ts, 0) == defaults[ts], "default tiles per group at %u bytes", ts);
		CHECK(adac::scan_tiles_per_group(ts, 1) == 1 && adac::scan_tiles_per_group(ts, 3) == 3, "the knob is not taken");
		CHECK((uint64_t)adac::scan_tiles_per_group(ts, 1000) * tile == adac::kDealMaxGroupRows, "the knob is not capped");
		for (int knob : {0, 1, 3, 1000}) {
			const int per = adac::scan_tiles_per_group(ts, knob);
			const uint32_t full = (uint32_t)per * tile;
			CHECK(adac::deal_scan_groups(ts, nullptr, nullptr, 0, true, per).empty(), "no segments yield groups");
			// a zero-row segment between two others
			std::vector<uint32_t> c = {tile + 5, 0, 77};
			std::vector<uint32_t> n = check_deal(ts, c, back_to_back(c), true, per);
			CHECK(n[1] == 0 && n[2] == 1, "zero-row segment: %u / %u groups", n[1], n[2]);
			// exactly `per` tiles, and `per` tiles + 1 row
			c = {full, full + 1};
			n = check_deal(ts, c, back_to_back(c), true, per);
			CHECK(n[0] == 1 && n[1] == 2, "%u and %u rows: %u and %u groups", full, full + 1, n[0], n[1]);
			// one row
			c = {1};
			n = check_deal(ts, c, back_to_back(c), true, per);
			CHECK(n[0] == 1, "one row: %u groups", n[0]);
			// many tiles, odd tails, starts off word boundaries
			c = {3, 5 * full + 17, 31, 2 * full, 1, 7 * tile - 1};
			check_deal(ts, c, back_to_back(c), true, per);
			// gapped value offsets: no cells
			std::vector<uint64_t> offs = {5, 5 + 3 * (uint64_t)full, (1ull << 33) + 1, (1ull << 33) + 4 * (uint64_t)full};
			c = {2 * full + 9, 40, full, 0};
			check_deal(ts, c, offs, false, per);
			// 40 one-row segments in a row, between two other segments: 26 and 16 arrivals at their two words
			c.assign(40, 1u);
			c.insert(c.begin(), 7u);
			c.push_back(2 * full + 3);
			n = check_deal(ts, c, back_to_back(c), true, per);
			CHECK(n[1] == 1 && n[40] == 1, "one-row segments");
			const std::vector<uint64_t> o = back_to_back(c);
			const std::vector<ScanGroupRef> refs = adac::deal_scan_groups(ts, c.data(), o.data(), c.size(), true, per);
			CHECK(refs[0].n_first == 26 && refs[1].n_first == 26 && refs[26].n_first == 16 && refs[41].n_first == 16,
			      "arrivals at the words of the one-row segments: %u %u %u %u", refs[0].n_first, refs[1].n_first,
			      refs[26].n_first, refs[41].n_first);
		}
	}
}

int main(int argc, char **argv) {
	if (argc == 3 && std::strcmp(argv[1], "per") == 0) {
		std::printf("%d\n", adac::scan_tiles_per_group((uint32_t)std::atoi(argv[2]), 0));
		return 0;
	}
	CHECK(argc == 1, "usage: %s [per TYPE_SIZE]", argv[0]);
	check_owner();
	check_groups();
	check_deals();
	std::printf("ok\n");
	return 0;
}
