// adac_bp_select_gather.inl — materialise only the rows a selection bitmap keeps, straight from DuckDB BITPACKING
// blocks (adac_bp_unpack_selected): the scan-with-selection half of ColumnSegment::FilterSelection for the persistent
// codec, the counterpart of adac_select_gather.inl.  Included into adac_kernels.hip after adac_bp_pair_scans.inl: the
// wave's run of groups, the mask window of a group (bp_group_window) and the kind dispatch are adac_bp_walk.inl's, the
// column cursor (BpCursor) is the pair scans'.
// Three steps, all on the device:
//   k_bp_group_popc  rows selected per metadata group (one wave per group, popcount over the group's mask window);
//   k_scan_*         adac_select_gather.inl's exclusive prefix (launch_exclusive_prefix) over the group table (group
//                    order = segment order = row order) -> each group's first output slot, and the grand total;
//   k_bp_gather      adac_bp_walk.inl's work shape: a WAVE walks a run of consecutive metadata groups on its own, one
//                    wave-private LDS stage.  Lane l of step k owns row 64 k + l; the selected lanes of a step store
//                    their values at CONSECUTIVE slots (slot = the group's running offset + the selected lanes
//                    below), so a step's stores are one contiguous run of the output.
// What is never read: a group without a selected row leaves on its count — no header, no mask word, no payload byte;
// a CONSTANT, CONSTANT_DELTA or width-0 group has no payload (the cursor's linear kind); in a FOR group a step whose
// mask word is zero is passed over, and with it every stage piece that holds such steps only.  A DELTA_FOR group is
// taken through its steps in order up to its last selected row: the prefix needs every row before that one.

struct BpGatherArgs {
	BpRun run;
	const uint8_t *blocks;
	const uint64_t *bitmap; // bit e = element out_off + row
	uint64_t tmask;         // all-ones of the type's width
	const uint32_t *group_cnt; // k_bp_group_popc's
	const uint64_t *group_off; // their exclusive prefix: the group's first output slot
};

// rows selected in each metadata group: one wave per group, four groups per workgroup
__global__ __launch_bounds__(kWorkgroup) void k_bp_group_popc(const BpGroup *__restrict__ groups, uint32_t ngroups,
                                                              const uint64_t *__restrict__ bitmap,
                                                              uint32_t *__restrict__ group_cnt) {
	const uint32_t gi = blockIdx.x * (kWorkgroup / 64) + (threadIdx.x >> 6);
	if (gi >= ngroups) return; // uniform per wave
	const uint32_t lane = threadIdx.x & 63u;
	const BpGroup g = groups[gi];
	const uint64_t win = bp_group_window<true>(g, bitmap, lane);
	const uint64_t c = wave_sum((uint64_t)__popcll(win));
	if (lane == 0) group_cnt[gi] = (uint32_t)c; // <= 2048
}

// One group, `left` > 0 of its rows selected, the first of them at slot `off`.
template <typename U, bool IDS, int KIND>
__device__ __forceinline__ void bp_gather_steps(BpCursor &c, uint64_t win, uint32_t lane, uint64_t off, uint32_t left,
                                                uint64_t elem0, U *__restrict__ out, uint64_t *__restrict__ out_ids) {
	const uint32_t steps = (c.n + 63u) >> 6;
	const uint64_t below = (1ull << lane) - 1ull;
	for (uint32_t k = 0; k < steps && left != 0u; k++) { // uniform; nothing selected after the last one: done
		const uint64_t wk = bp_readlane64(win, k);
		// nothing of the step is wanted: legal to pass over only when no prefix has to advance
		if (KIND != kBpCurDelta && wk == 0ull) continue;
		const uint64_t v = bp_cursor_value<KIND>(c, k, lane);
		if ((wk >> lane) & 1ull) { // never a row past the group: the window is cut to its rows
			const uint64_t slot = off + (uint32_t)__popcll(wk & below);
			out[slot] = (U)v;
			if (IDS) out_ids[slot] = elem0 + k * 64u + lane;
		}
		const uint32_t here = (uint32_t)__popcll(wk);
		off += here;
		left -= here;
	}
}

template <typename U, bool IDS>
__global__ __launch_bounds__(kWorkgroup) void k_bp_gather(const BpGroup *__restrict__ groups, const BpGatherArgs s,
                                                          U *__restrict__ out, uint64_t *__restrict__ out_ids) {
	__shared__ uint4 lds[kBpWaves * kBpScanWaveChunks];
	const BpWaveRun w(s.run, lds, 1);
	if (w.none) return;
	const uint32_t lane = w.lane;
	for (uint32_t gi = w.g0; gi < w.g1; gi++) {
		const uint32_t cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.group_cnt[gi]);
		if (cnt == 0u) continue; // nothing selected here: neither the header nor a mask word nor the payload is read
		const uint64_t off = s.group_off[gi];
		const BpGroup g = groups[gi];
		BpCursor c;
		const int kind = bp_cursor_open(c, g, s.blocks, s.tmask, w.stage);
		const uint64_t win = bp_group_window<true>(g, s.bitmap, lane);
		bp_with_kind(kind, [&](auto tk) __attribute__((always_inline)) {
			bp_gather_steps<U, IDS, decltype(tk)::value>(c, win, lane, off, cnt, g.out_off, out, out_ids);
		});
	}
}
