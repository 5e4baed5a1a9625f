// adac_bp_walk.inl — what the wave-per-run kernels on DuckDB BITPACKING blocks share: k_bp_scan (adac_bp_scans.inl),
// k_bp_scan_pair_sum, k_bp_scan_pair_gsum and k_bp_scan_pair_cmp (adac_bp_pair_scans.inl), k_bp_gather and
// k_bp_group_popc (adac_bp_select_gather.inl).  Included into adac_kernels.hip after adac_bitpacking.inl (the BpGroup
// table filled by k_bp_prepare) and before those three.
//
// Work shape: a WAVE walks a run of `per_wave` consecutive metadata groups on its own — no barrier anywhere.  Lane l
// of step k owns row 64 k + l of the group, so a step's fields are 64 neighbours of the bit stream and its mask bits
// ONE 64-bit window of the validity / selection mask.  The pieces:
//   BpRun, BpWaveRun  the run's description in the kernel arguments (bp_wave_grid in adac_kernels.hip sizes it) and
//                     the wave's part of it: groups [g0, g1), the lane, the wave's LDS stage buffers
//   bp_group_window   lane j: which of the rows [64 j, 64 j + 64) of a group exist and are wanted
//   bp_group_emit     the other way round: lane j's ballot of step j into the group's words of a selection bitmap
//   bp_stage_piece    payload rows [r0, r1) of a group into a wave-private LDS buffer of at most 4 KiB of payload: a
//                     group wider than 16 bits is staged in pieces of whole steps (bp_stage_rows)
//   bp_with_kind      how a group's values are had (linear / FOR / DELTA) as a compile-time constant

constexpr uint32_t kBpWaves = kWorkgroup / 64;
constexpr uint32_t kBpScanStageBytes = 4096;                     // payload bytes a wave stages at a time
constexpr uint32_t kBpScanWaveChunks = kBpScanStageBytes / 16 + 3; // + the start's misalignment + read_field's over-read
constexpr uint32_t kBpScanStageLoads = (kBpScanStageBytes / 16 + 1 + 63) / 64;

// head of the kernels' argument structs
struct BpRun {
	uint32_t ngroups;
	uint32_t per_wave; // consecutive groups one wave walks
};

// A wave's part of the run.  lds: kBpWaves * nstage * kBpScanWaveChunks chunks.
struct BpWaveRun {
	uint32_t wave; // of the workgroup's kBpWaves, uniform
	uint32_t lane;
	bool none;       // no group is left for this wave (uniform): the kernels return, no barrier follows
	uint32_t g0, g1; // else the wave's groups
	uint4 *stage;    // the wave's `nstage` buffers of kBpScanWaveChunks chunks each, one behind the other
	__device__ __forceinline__ BpWaveRun(const BpRun &r, uint4 *lds, uint32_t nstage) {
		wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
		lane = threadIdx.x & 63u;
		const uint64_t first = ((uint64_t)blockIdx.x * kBpWaves + wave) * r.per_wave;
		none = first >= r.ngroups;
		g0 = (uint32_t)first;
		g1 = first + r.per_wave < r.ngroups ? g0 + r.per_wave : r.ngroups;
		stage = lds + wave * nstage * kBpScanWaveChunks;
	}
};

__device__ __forceinline__ uint64_t bp_readlane64(uint64_t v, uint32_t k /* uniform */) {
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)k);
	const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)k);
	return ((uint64_t)hi << 32) | lo;
}

// lane j: which of the rows [64 j, 64 j + 64) of the group exist and, <V>, have their bit set in `mask` (bit e =
// element out_off + row): one 64-bit funnel of two neighbouring mask words per lane
template <bool V>
__device__ __forceinline__ uint64_t bp_group_window(const BpGroup &g, const uint64_t *mask, uint32_t lane) {
	const uint32_t n = g.rows;
	const uint32_t left = 64u * lane < n ? n - 64u * lane : 0u;
	uint64_t win = left >= 64u ? ~0ull : ((1ull << left) - 1ull);
	if (V) {
		const uint32_t sh = (uint32_t)(g.out_off & 63u);
		const uint64_t word0 = g.out_off >> 6;
		const uint32_t nwords = (uint32_t)(((g.out_off + n - 1u) >> 6) - word0) + 1u; // <= 33
		const uint64_t vw = lane < nwords ? mask[word0 + lane] : 0ull;
		const uint64_t nx = __shfl_down(vw, 1, 64);
		win &= sh ? (vw >> sh) | (nx << (64u - sh)) : vw;
	}
	return win;
}

// lane j holds the hits of step j (rows [64 j, 64 j + 64) of a group of n rows, bit e = element out_off + row): the
// group's words of the zeroed `bitmap`, as bp_group_window takes them from a mask.  Words wholly inside the group are
// stored, its first and last go through atomicOr: neighbouring groups and segments may share them at any bit phase.
__device__ __forceinline__ void bp_group_emit(uint64_t out_off, uint32_t n, uint64_t hits, unsigned long long *bitmap,
                                              uint32_t lane) {
	const uint32_t sh = (uint32_t)(out_off & 63u);
	const uint64_t word0 = out_off >> 6;
	const uint32_t nwords = (uint32_t)(((out_off + n - 1u) >> 6) - word0) + 1u; // <= 33
	// word j of the group holds the rows [64 j - sh, 64 j - sh + 64): the top of step j - 1, the bottom of step j
	uint64_t prev = __shfl_up(hits, 1, 64);
	if (lane == 0) prev = 0ull;
	const uint64_t word = sh ? (hits << sh) | (prev >> (64u - sh)) : hits;
	if (lane < nwords && word != 0ull) {
		if (lane == 0 || lane == nwords - 1u) {
			atomicOr(bitmap + word0 + lane, (unsigned long long)word);
		} else {
			bitmap[word0 + lane] = word;
		}
	}
}

// rows of one staged piece: the whole group up to 16 bits, else the whole steps that fit kBpScanStageBytes
__device__ __forceinline__ uint32_t bp_stage_rows(uint32_t w) {
	return w <= 16u ? (uint32_t)kBpGroupRows : ((kBpScanStageBytes * 8u / w) & ~63u);
}

// Stage the piece that starts at row r0 (a multiple of stage_rows = bp_stage_rows(w), which the callers step by) of a
// group of n rows at width w >= 1 whose payload starts pbit bits into the 16-byte chunk src16: aligned 16-byte loads,
// the index clamped to the piece's last chunk.  r1: the piece's end; bit0: row r0's bit in the staged image.
// Everything but `lane` is uniform.
// LDS operations of one wave execute in order.  The first fence keeps the stores behind every read of the piece that
// was resident before (the caller's, earlier in the program: k_bp_scan's last piece, a cursor's any earlier one); the
// second keeps the caller's reads behind the stores.  The first is right on either side of the loads, and each caller
// keeps the side it had and is faster with (profiles/r09_bp_walk_refactor.json): k_bp_scan in front of them
// (FENCE_LOADS = false), the cursors behind them (true).
template <bool FENCE_LOADS>
__device__ __forceinline__ void bp_stage_piece(const uint4 *src16, uint32_t pbit, uint32_t w, uint32_t n,
                                               uint32_t stage_rows, uint32_t r0, uint4 *stage, uint32_t lane,
                                               uint32_t &r1, uint32_t &bit0) {
	r1 = r0 + stage_rows < n ? r0 + stage_rows : n;
	const uint32_t bits = pbit + r0 * w;
	const uint4 *src = src16 + (bits >> 7);
	bit0 = bits & 127u;
	const uint32_t nchunks = (bit0 + (r1 - r0) * w + 127u) >> 7; // <= kBpScanStageBytes / 16 + 1
	uint4 q[kBpScanStageLoads];
	if (!FENCE_LOADS) __builtin_amdgcn_wave_barrier();
#pragma unroll
	for (uint32_t i = 0; i < kBpScanStageLoads; i++) { // all requested before the first is stored
		const uint32_t c = lane + 64u * i;
		q[i] = make_uint4(0u, 0u, 0u, 0u);
		if (64u * i < nchunks) q[i] = src[c < nchunks ? c : nchunks - 1u]; // uniform test, index clamped
	}
	if (FENCE_LOADS) __builtin_amdgcn_wave_barrier();
#pragma unroll
	for (uint32_t i = 0; i < kBpScanStageLoads; i++) {
		const uint32_t c = lane + 64u * i;
		if (c < nchunks) stage[c] = q[i];
	}
	__builtin_amdgcn_wave_barrier();
}

// How a group's values are had: see BpCursor in adac_bp_pair_scans.inl
enum : int { kBpCurLinear = 0, kBpCurFor = 1, kBpCurDelta = 2 };

// f(std::integral_constant<int, kind>); the callers pass a generic lambda marked always_inline
template <typename F>
__device__ __forceinline__ void bp_with_kind(int kind /* uniform */, F &&f) {
	if (kind == kBpCurLinear) f(std::integral_constant<int, kBpCurLinear> {});
	else if (kind == kBpCurFor) f(std::integral_constant<int, kBpCurFor> {});
	else f(std::integral_constant<int, kBpCurDelta> {});
}
