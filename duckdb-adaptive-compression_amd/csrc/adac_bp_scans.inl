// adac_bp_scans.inl — fused filter / aggregate scans on DuckDB BITPACKING blocks: SUM, COUNT / select BETWEEN and
// MIN / MAX per segment straight from the block images, under an optional validity mask, nothing decoded to HBM.
// Included into adac_kernels.hip after adac_bp_walk.inl: the wave's run of groups, the mask window of a group and
// the staging of its payload are written there; the BpGroup table filled by k_bp_prepare, read_field and
// wave_inclusive_sum are shared with the decode (adac_bitpacking.inl).  Every result equals the same aggregate over
// what k_bp_unpack writes for these bytes (value = T(field + frame) wrapping in T, DELTA_FOR prefix wrapping in T):
// shortcuts are taken only where that is provable.
//
// Work shape (adac_bp_walk.inl): lane l of step k owns row 64 k + l of the group, so
//   * a step's fields are 64 neighbours of the bit stream (conflict-free LDS reads of the wave's stage);
//   * the mask bits of a step are ONE 64-bit window of the validity mask and its hits ONE ballot: lane k keeps the
//     window / the ballot of step k, and a group's bitmap words leave with one store per lane;
//   * DELTA_FOR is one DPP wave scan per step, carried from step to step in a uniform register; every row of the
//     group is part of the prefix, masked or not.
// Per metadata group:
//   CONSTANT, FOR at width 0      no payload byte read: SUM = widen(c) * popcount(mask), select = the mask or nothing
//   CONSTANT_DELTA, DELTA_FOR w 0 T(a + i * step) from the row index, no payload byte read
//   FOR                           COUNT / select: [frame, frame + 2^w) against [lo, hi] in T's ordered domain when
//                                 the interval does not wrap there — disjoint: nothing; inside: the mask bits; neither
//                                 reads payload.  Otherwise (and for SUM, MIN / MAX) row by row.
//   DELTA_FOR                     row by row behind the prefix
// Results: the caller fills sums / counts with zero, min / max (in the ordered domain bits ^ signbit) with the empty
// interval and the bitmap with zero; a wave adds what it gathered over the groups of ONE segment with one 64-bit
// atomic per result (k_scan_product's scheme).  Bitmap words wholly inside a group are stored, a group's first and
// last word go through atomicOr: neighbouring groups and segments may share them at any bit phase.

enum : int { kBpScanSum = 0, kBpScanRange = 1, kBpScanMinMax = 2 };

struct BpScanArgs {
	BpRun run;
	const uint8_t *blocks;
	const uint64_t *validity; // bit e = element out_off + row; read only by the <V> kernels
	uint64_t sbit;            // T's sign bit, 0 for the unsigned types
	uint64_t blo, bspan;      // range scans: lo and hi - lo in the ordered domain
	unsigned long long *res;  // sums | counts | min, max pairs in the ordered domain
	unsigned long long *bitmap; // select; nullptr: count only
};

// what a lane gathered over the groups of one segment
template <int OP>
struct BpScanAcc {
	uint64_t a = OP == kBpScanMinMax ? ~0ull : 0ull; // sum | count | min (ordered)
	uint64_t b = 0ull;                               // max (ordered)
	__device__ __forceinline__ void flush(unsigned long long *res, uint32_t seg, uint32_t lane) {
		if (OP == kBpScanMinMax) {
			const uint64_t mn = wave_min(a), mx = wave_max(b);
			if (lane == 0 && mn <= mx) {
				atomicMin(res + 2 * (uint64_t)seg, (unsigned long long)mn);
				atomicMax(res + 2 * (uint64_t)seg + 1, (unsigned long long)mx);
			}
			a = ~0ull;
			b = 0ull;
		} else {
			const uint64_t t = wave_sum(a);
			if (lane == 0 && t != 0ull) atomicAdd(res + seg, (unsigned long long)t);
			a = 0ull;
		}
	}
	// the walk reaches a group of segment gs: what was gathered over another segment leaves first
	__device__ __forceinline__ void enter(uint32_t gs, uint32_t &seg, unsigned long long *res, uint32_t lane) {
		if (gs != seg) {
			flush(res, seg, lane);
			seg = gs;
		}
	}
};

// One row per lane of step k: `keep` = the row exists and its mask bit is set.  `hits`: lane k keeps step k's ballot.
template <typename U, int OP>
__device__ __forceinline__ void bp_scan_row(const BpScanArgs &s, uint32_t k, uint32_t lane, U val, bool keep,
                                            BpScanAcc<OP> &acc, uint64_t &hits) {
	if (OP == kBpScanSum) {
		const uint64_t wide = ((uint64_t)val ^ s.sbit) - s.sbit; // widened by T's signedness
		acc.a += keep ? wide : 0ull;
	} else if (OP == kBpScanRange) {
		const U d = (U)((U)(val ^ (U)s.sbit) - (U)s.blo);
		const uint64_t ballot = __ballot(keep && d <= (U)s.bspan);
		if (lane == k) hits = ballot;
	} else {
		const uint64_t o = (uint64_t)val ^ s.sbit;
		if (keep) {
			acc.a = o < acc.a ? o : acc.a;
			acc.b = o > acc.b ? o : acc.b;
		}
	}
}

// FOR / DELTA_FOR at width >= 1: the payload piece by piece (bp_stage_piece) through the wave's LDS buffer.
// SCAN32 (DELTA_FOR of a 64-bit type at w <= 26): the fields of a step sum to less than 2^32, so the wave scan runs
// on one dword.
template <typename U, int OP, bool V, bool WIDE, bool DELTA, bool SCAN32 = false>
__device__ __forceinline__ void bp_scan_packed(const BpScanArgs &s, const BpGroup &g, uint4 *stage, uint32_t lane,
                                               uint64_t win, BpScanAcc<OP> &acc, uint64_t &hits) {
	const uint32_t n = g.rows, w = g.width;
	const uint32_t mlo = WIDE ? 0xffffffffu : mask32(w);
	const uint32_t mhi = WIDE ? mask32(w - 32u) : 0u;
	const uintptr_t addr = reinterpret_cast<uintptr_t>(s.blocks + g.payload_off);
	const uint4 *src16 = reinterpret_cast<const uint4 *>(addr & ~uintptr_t(15));
	const uint32_t pbit = (uint32_t)(addr & 15) * 8u;
	const uint32_t stage_rows = bp_stage_rows(w);
	const uint32_t *lds32 = reinterpret_cast<const uint32_t *>(stage);
	const U frame = (U)g.frame;
	// DELTA_FOR: v[i] = delta_offset + (i + 1) * frame + sum_{j <= i} field[j], all mod 2^bits; `base` is the part of
	// it that the rows before the step contribute
	U base = (U)g.extra;
	const U lane_frames = (U)((U)(lane + 1u) * frame);
	for (uint32_t r0 = 0; r0 < n; r0 += stage_rows) { // uniform
		uint32_t r1, bit0;
		bp_stage_piece<false>(src16, pbit, w, n, stage_rows, r0, stage, lane, r1, bit0);
		uint32_t fbit = bit0 + lane * w; // of the lane's row in the staged image: 64 rows further every step
#pragma unroll 2
		for (uint32_t k = r0 >> 6; k * 64u < r1; k++, fbit += 64u * w) {
			const uint64_t wk = bp_readlane64(win, k);
			if (V && !DELTA && wk == 0ull) continue; // nothing of the step is wanted
			const uint32_t row = k * 64u + lane;
			const bool keep = (wk >> lane) & 1ull;
			uint32_t lo, hi;
			read_field<WIDE>(lds32, row < r1 ? fbit : bit0, mlo, mhi, lo, hi); // clamped into the stage
			U val;
			if (DELTA) {
				const U f = row < n ? (sizeof(U) == 8 ? (U)(((uint64_t)hi << 32) | lo) : (U)lo) : (U)0;
				const U incl = SCAN32 ? (U)wave_inclusive_sum<uint32_t>((uint32_t)f) : wave_inclusive_sum<U>(f);
				val = (U)(base + lane_frames + incl);
				const U total = sizeof(U) == 8 ? (U)bp_readlane64((uint64_t)incl, 63u)
				                               : (U)__builtin_amdgcn_readlane((int)(uint32_t)incl, 63);
				base = (U)(base + (U)(64u * frame) + total);
			} else {
				val = sizeof(U) == 8 ? (U)((((uint64_t)hi << 32) | lo) + g.frame) : (U)(lo + (uint32_t)g.frame);
			}
			bp_scan_row<U, OP>(s, k, lane, val, keep, acc, hits);
		}
	}
}

template <typename U, int OP, bool V>
__device__ __forceinline__ void bp_scan_group(const BpScanArgs &s, const BpGroup &g, uint4 *stage, uint32_t lane,
                                              BpScanAcc<OP> &acc) {
	const uint32_t n = g.rows;
	const uint64_t win = bp_group_window<V>(g, s.validity, lane);
	const uint64_t tmask = (uint64_t)(U)~(U)0;
	const uint32_t steps = (n + 63u) >> 6;
	uint64_t hits = 0ull;
	const bool packed = (g.mode == kBpFor || g.mode == kBpDeltaFor) && g.width != 0u;
	if (!packed) {
		// v[i] = first + i * step (k_bp_unpack's width-0 branch); step 0: CONSTANT and FOR at width 0
		U first = (U)g.frame, step = (U)0;
		if (g.mode == kBpConstantDelta) step = (U)g.extra;
		if (g.mode == kBpDeltaFor) {
			first = (U)((U)g.extra + (U)g.frame);
			step = (U)g.frame;
		}
		if (step == (U)0) {
			const uint64_t o = (uint64_t)first ^ s.sbit;
			if (OP == kBpScanSum) {
				acc.a += (o - s.sbit) * (uint64_t)__popcll(win);
			} else if (OP == kBpScanRange) {
				hits = (U)((U)o - (U)s.blo) <= (U)s.bspan ? win : 0ull;
			} else if (win != 0ull) {
				acc.a = o < acc.a ? o : acc.a;
				acc.b = o > acc.b ? o : acc.b;
			}
		} else {
			for (uint32_t k = 0; k < steps; k++) {
				const uint64_t wk = bp_readlane64(win, k);
				const uint32_t row = k * 64u + lane;
				bp_scan_row<U, OP>(s, k, lane, (U)(first + (U)((U)row * step)), (wk >> lane) & 1ull, acc, hits);
			}
		}
	} else {
		bool walk = true;
		if (OP == kBpScanRange && g.mode == kBpFor) {
			// ordered(field + frame) = field + ordered(frame) as long as that stays inside T's ordered domain
			const uint64_t olo = (g.frame & tmask) ^ s.sbit, span = mask64(g.width);
			const uint64_t bhi = s.blo + s.bspan;
			if (span <= tmask - olo) {
				const uint64_t ohi = olo + span;
				if (ohi < s.blo || olo > bhi) {
					walk = false; // the group's interval misses [lo, hi]
				} else if (olo >= s.blo && ohi <= bhi) {
					hits = win; // inside: every wanted row
					walk = false;
				}
			}
		}
		if (walk) {
			const bool wide = sizeof(U) == 8 && g.width > 32u;
			if (g.mode == kBpFor) {
				if (wide) bp_scan_packed<U, OP, V, sizeof(U) == 8, false>(s, g, stage, lane, win, acc, hits);
				else bp_scan_packed<U, OP, V, false, false>(s, g, stage, lane, win, acc, hits);
			} else {
				if (wide) bp_scan_packed<U, OP, V, sizeof(U) == 8, true>(s, g, stage, lane, win, acc, hits);
				else if (sizeof(U) == 8 && g.width <= 26u) bp_scan_packed<U, OP, V, false, true, sizeof(U) == 8>(s, g, stage, lane, win, acc, hits);
				else bp_scan_packed<U, OP, V, false, true>(s, g, stage, lane, win, acc, hits);
			}
		}
	}
	if (OP == kBpScanRange) {
		acc.a += (uint64_t)__popcll(hits);
		if (s.bitmap != nullptr) bp_group_emit(g.out_off, n, hits, s.bitmap, lane);
	}
}

template <typename U, int OP, bool V>
__global__ __launch_bounds__(kWorkgroup) void k_bp_scan(const BpGroup *__restrict__ groups,
                                                        const uint32_t *__restrict__ group_seg /* of every group */,
                                                        const BpScanArgs s) {
	__shared__ uint4 lds[kBpWaves * kBpScanWaveChunks];
	const BpWaveRun w(s.run, lds, 1);
	if (w.none) return;
	BpScanAcc<OP> acc;
	uint32_t seg = group_seg[w.g0];
	for (uint32_t gi = w.g0; gi < w.g1; gi++) {
		acc.enter(group_seg[gi], seg, s.res, w.lane);
		const BpGroup g = groups[gi];
		bp_scan_group<U, OP, V>(s, g, w.stage, w.lane, acc);
	}
	acc.flush(s.res, seg, w.lane);
}

// min / max cells from the ordered domain back to T's bits; a segment without a selected row reports the empty
// interval [T's maximum, T's minimum] (adac_zonemap's convention)
__global__ void k_bp_scan_minmax_finish(uint64_t *__restrict__ minmax, uint64_t nseg, uint64_t tmask, uint64_t sbit) {
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nseg) return;
	const uint64_t mn = minmax[2 * i], mx = minmax[2 * i + 1];
	const bool empty = mn > mx;
	minmax[2 * i] = (empty ? tmask : mn) ^ sbit;
	minmax[2 * i + 1] = (empty ? 0ull : mx) ^ sbit;
}
