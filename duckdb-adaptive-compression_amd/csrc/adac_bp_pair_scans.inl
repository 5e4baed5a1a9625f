// adac_bp_pair_scans.inl — fused scans over TWO columns of DuckDB BITPACKING blocks walked in step: SUM(a * b) per
// segment (Q6's aggregate), SUM(v), COUNT(*) GROUP BY key (Q1's basic shape) and the selection of the rows where
// a <cmp> b (Q12's l_commitdate < l_receiptdate), under an optional selection bitmap, nothing decoded to HBM.
// Included into adac_kernels.hip after adac_bp_scans.inl: the wave's run of groups, the mask window of a group, the
// staging of a piece, the kind dispatch and the bitmap words of a group are adac_bp_walk.inl's, BpScanAcc is
// k_bp_scan's.
//
// Work shape (adac_bp_walk.inl): a WAVE walks a run of consecutive metadata groups on its own.  The host has checked
// that group i of both layouts covers the same rows at the same element offset, so the wave takes group i of both
// columns; lane l of step k owns row 64 k + l of both, and the mask bits of a step are one 64-bit window in the FIRST
// layout's element space.
//
// A column is read through a cursor (BpCursor) that yields the lane's value of step k as 64 bits masked to the type's
// width (the prefix mod 2^64 and then mod 2^bits is the prefix mod 2^bits), so one kernel serves every pair of types:
//   linear   CONSTANT, CONSTANT_DELTA, FOR / DELTA_FOR at width 0: first + row * step, no payload byte read
//   FOR      field + frame
//   DELTA    the running prefix: one DPP wave scan per step, carried in a uniform register.  EVERY step of the group
//            must pass through the cursor in order, masked or not.
// The kind is a template parameter of the step loop (nine pairs), the width is not: a field is read branch-free as
// three dwords.  Each cursor stages its payload through a wave-private LDS buffer of its own, in pieces of whole
// steps when the width is above 16; which piece is resident is decided by the STEP INDEX asked for (the pieces of a
// 21-bit and of a 40-bit column end at different steps, and steps whose mask window is zero are skipped when neither
// column is DELTA).
// Results: the caller zeroes them.  SUM(a * b): a wave adds what it gathered over the groups of one segment of the
// first layout with one 64-bit atomic.  Grouped: bins live in LDS per wave — 16 / 8 / 4 / 2 / 1 copies of the
// ngroups + 1 bins, lane & (copies - 1) picks one, so few lanes collide on an LDS add when there are few keys — and at
// its end the wave touches every bin with one global atomic.  A group whose key column is a constant updates its bin
// once.  Compare: counts per segment as SUM(a * b)'s sums; one ballot per step, and a group's words of the bitmap
// leave as k_bp_scan's do (bp_group_emit).  The values are compared as mathematical integers (BpMath), so the two
// types may differ in width and signedness.  What only a group's end needs waits in vector registers (bp_park).

constexpr uint32_t kBpPairBins = 257; // 256 groups + overflow

struct BpPairArgs {
	BpRun run; // metadata groups: the same number in both layouts
	const uint8_t *a_blocks, *b_blocks;
	const uint64_t *validity; // bit e = element out_off + row of the first layout; read only by the <V> kernels
	uint64_t a_tmask, a_sbit, b_tmask, b_sbit; // all-ones of the type's width; its sign bit, 0 for the unsigned types
	unsigned long long *res;    // sums per segment of the first layout | sums per key
	unsigned long long *counts; // grouped: rows per key, or nullptr
	uint32_t nkeys;             // grouped: keys >= nkeys land in bin nkeys
};

// Every member is wave-uniform and lives in scalar registers: only what cannot be had from the width in a few
// scalar instructions is kept (two cursors, the mask window and the bins share ~100 of them).
struct BpCursor {
	const uint4 *src16; // the 16-byte chunk holding the payload's first byte
	uint4 *stage;       // kBpScanWaveChunks chunks of LDS, this wave's and this column's
	uint64_t frame;     // linear: the first value.  FOR / DELTA: the frame of reference
	uint64_t base;      // linear: the step.  DELTA: what the rows before the current step contribute
	uint64_t tmask;
	uint32_t n, w, pbit;
	uint32_t r0, r1, bit0; // the resident piece: rows [r0, r1), row r0's bit in the staged image
};

__device__ __forceinline__ int bp_cursor_open(BpCursor &c, const BpGroup &g, const uint8_t *blocks, uint64_t tmask,
                                              uint4 *stage) {
	c.tmask = tmask;
	c.n = g.rows;
	c.stage = stage;
	c.w = g.width;
	c.src16 = nullptr;
	c.pbit = c.r0 = c.r1 = c.bit0 = 0u;
	if ((g.mode != kBpFor && g.mode != kBpDeltaFor) || g.width == 0u) {
		// v[i] = first + i * step (k_bp_unpack's width-0 branch); step 0: CONSTANT and FOR at width 0
		c.frame = g.frame;
		c.base = 0ull;
		if (g.mode == kBpConstantDelta) c.base = g.extra & tmask;
		if (g.mode == kBpDeltaFor) {
			c.frame = g.extra + g.frame;
			c.base = g.frame & tmask;
		}
		return kBpCurLinear;
	}
	const uintptr_t addr = reinterpret_cast<uintptr_t>(blocks + g.payload_off);
	c.src16 = reinterpret_cast<const uint4 *>(addr & ~uintptr_t(15));
	c.pbit = (uint32_t)(addr & 15) * 8u;
	c.frame = g.frame;
	c.base = g.extra;
	return g.mode == kBpFor ? kBpCurFor : kBpCurDelta;
}

// Make the piece that holds step k resident.
__device__ __forceinline__ void bp_cursor_stage(BpCursor &c, uint32_t k /* uniform */, uint32_t lane) {
	const uint32_t stage_rows = bp_stage_rows(c.w);
	c.r0 = (k * 64u / stage_rows) * stage_rows;
	bp_stage_piece<true>(c.src16, c.pbit, c.w, c.n, stage_rows, c.r0, c.stage, lane, c.r1, c.bit0);
}

// The lane's value of step k, masked to the type's width.  DELTA: call for every k = 0, 1, 2 ... of the group.
template <int KIND>
__device__ __forceinline__ uint64_t bp_cursor_value(BpCursor &c, uint32_t k /* uniform */, uint32_t lane) {
	const uint32_t row = k * 64u + lane;
	if (KIND == kBpCurLinear) return (c.frame + (uint64_t)row * c.base) & c.tmask;
	if (k * 64u < c.r0 || k * 64u >= c.r1) bp_cursor_stage(c, k, lane); // never resident at first: r0 = r1 = 0
	// rows past the group are clamped into the stage; the third dword lies inside the stage's spare chunks
	const uint32_t bit = row < c.r1 ? c.bit0 + (row - c.r0) * c.w : c.bit0;
	const uint32_t *lds32 = reinterpret_cast<const uint32_t *>(c.stage);
	const uint32_t dw = bit >> 5, sh = bit & 31u;
	const uint32_t a0 = lds32[dw], a1 = lds32[dw + 1], a2 = lds32[dw + 2];
	const uint32_t lo = __builtin_amdgcn_alignbit(a1, a0, sh) & mask32(c.w);
	const uint32_t hi = __builtin_amdgcn_alignbit(a2, a1, sh) & (c.w > 32u ? mask32(c.w - 32u) : 0u);
	uint64_t f = ((uint64_t)hi << 32) | lo;
	if (KIND == kBpCurFor) return (f + c.frame) & c.tmask;
	// v[i] = delta_offset + (i + 1) * frame + sum_{j <= i} field[j]
	f = row < c.n ? f : 0ull;
	uint64_t incl;
	// on one dword where that is exact: a type of at most 32 bits wraps there anyway, and 64 fields of at most 26 bits
	// sum to less than 2^32
	if (c.tmask <= 0xffffffffull || c.w <= 26u) incl = (uint64_t)wave_inclusive_sum<uint32_t>((uint32_t)f);
	else incl = wave_inclusive_sum<uint64_t>(f);
	const uint64_t val = c.base + (uint64_t)(lane + 1u) * c.frame + incl;
	c.base += 64ull * c.frame + bp_readlane64(incl, 63u);
	return val & c.tmask;
}

__device__ __forceinline__ uint64_t bp_widen(uint64_t v, uint64_t sbit) { return (v ^ sbit) - sbit; }

// ---- SUM(a * b) -----------------------------------------------------------------------------------------------

template <int KA, int KB>
__device__ __forceinline__ void bp_pair_sum_steps(const BpPairArgs &s, BpCursor &ca, BpCursor &cb, uint64_t win,
                                                  uint32_t lane, BpScanAcc<kBpScanSum> &acc) {
	if (KA == kBpCurLinear && KB == kBpCurLinear && ca.base == 0ull && cb.base == 0ull) { // two constants
		acc.a += bp_widen(ca.frame & ca.tmask, s.a_sbit) * bp_widen(cb.frame & cb.tmask, s.b_sbit) *
		         (uint64_t)__popcll(win);
		return;
	}
	const uint32_t steps = (ca.n + 63u) >> 6;
	for (uint32_t k = 0; k < steps; k++) {
		const uint64_t wk = bp_readlane64(win, k);
		// nothing of the step is wanted: legal to pass over only when no prefix has to advance
		if (KA != kBpCurDelta && KB != kBpCurDelta && wk == 0ull) continue;
		const uint64_t va = bp_cursor_value<KA>(ca, k, lane);
		const uint64_t vb = bp_cursor_value<KB>(cb, k, lane);
		const uint64_t p = bp_widen(va, s.a_sbit) * bp_widen(vb, s.b_sbit);
		acc.a += ((wk >> lane) & 1ull) ? p : 0ull;
	}
}

template <bool V>
__global__ __launch_bounds__(kWorkgroup) void k_bp_scan_pair_sum(const BpGroup *__restrict__ a_groups,
                                                                 const BpGroup *__restrict__ b_groups,
                                                                 const uint32_t *__restrict__ group_seg /* of a */,
                                                                 const BpPairArgs s) {
	__shared__ uint4 lds[kBpWaves * 2 * kBpScanWaveChunks];
	const BpWaveRun w(s.run, lds, 2);
	if (w.none) return;
	const uint32_t lane = w.lane;
	BpScanAcc<kBpScanSum> acc;
	uint32_t seg = group_seg[w.g0];
	for (uint32_t gi = w.g0; gi < w.g1; gi++) {
		acc.enter(group_seg[gi], seg, s.res, lane);
		const BpGroup ga = a_groups[gi], gb = b_groups[gi];
		BpCursor ca, cb;
		const int ka = bp_cursor_open(ca, ga, s.a_blocks, s.a_tmask, w.stage);
		const int kb = bp_cursor_open(cb, gb, s.b_blocks, s.b_tmask, w.stage + kBpScanWaveChunks);
		const uint64_t win = bp_group_window<V>(ga, s.validity, lane);
		bp_with_kind(ka, [&](auto ta) __attribute__((always_inline)) {
			bp_with_kind(kb, [&](auto tb) __attribute__((always_inline)) {
				bp_pair_sum_steps<decltype(ta)::value, decltype(tb)::value>(s, ca, cb, win, lane, acc);
			});
		});
	}
	acc.flush(s.res, seg, lane);
}

// ---- SUM(v), COUNT(*) GROUP BY key ----------------------------------------------------------------------------

struct BpPairBins {
	unsigned long long *sums, *counts; // this wave's: kBpPairBins words each
	uint32_t copies;                   // power of two; bin b's copies at [b * copies, (b + 1) * copies)
};

// the key column is a constant over the group: the lanes gather, one bin update per group
template <int KV>
__device__ __forceinline__ void bp_pair_gsum_one_key(const BpPairArgs &s, BpCursor &cv, uint64_t key, uint64_t win,
                                                     uint32_t lane, const BpPairBins &bins) {
	uint64_t sum = 0ull;
	if (KV == kBpCurLinear && cv.base == 0ull) {
		sum = bp_widen(cv.frame & cv.tmask, s.a_sbit) * (uint64_t)__popcll(win);
	} else {
		const uint32_t steps = (cv.n + 63u) >> 6;
		for (uint32_t k = 0; k < steps; k++) {
			const uint64_t wk = bp_readlane64(win, k);
			if (KV != kBpCurDelta && wk == 0ull) continue;
			const uint64_t v = bp_cursor_value<KV>(cv, k, lane);
			sum += ((wk >> lane) & 1ull) ? bp_widen(v, s.a_sbit) : 0ull;
		}
	}
	sum = wave_sum(sum);
	const uint64_t cnt = wave_sum((uint64_t)__popcll(win));
	const uint32_t bin = key < (uint64_t)s.nkeys ? (uint32_t)key : s.nkeys;
	if (lane == 0 && cnt != 0ull) {
		atomicAdd(bins.sums + bin * bins.copies, (unsigned long long)sum);
		atomicAdd(bins.counts + bin * bins.copies, (unsigned long long)cnt);
	}
}

template <int KV, int KK>
__device__ __forceinline__ void bp_pair_gsum_steps(const BpPairArgs &s, BpCursor &cv, BpCursor &ck, uint64_t win,
                                                   uint32_t lane, const BpPairBins &bins) {
	if (KK == kBpCurLinear && ck.base == 0ull) {
		bp_pair_gsum_one_key<KV>(s, cv, ck.frame & ck.tmask, win, lane, bins);
		return;
	}
	const uint32_t steps = (cv.n + 63u) >> 6;
	const uint32_t copy = lane & (bins.copies - 1u);
	for (uint32_t k = 0; k < steps; k++) {
		const uint64_t wk = bp_readlane64(win, k);
		if (KV != kBpCurDelta && KK != kBpCurDelta && wk == 0ull) continue;
		const uint64_t v = bp_cursor_value<KV>(cv, k, lane);
		const uint64_t key = bp_cursor_value<KK>(ck, k, lane); // unsigned, of the key type's own width
		const uint32_t bin = key < (uint64_t)s.nkeys ? (uint32_t)key : s.nkeys;
		if ((wk >> lane) & 1ull) {
			atomicAdd(bins.sums + bin * bins.copies + copy, (unsigned long long)bp_widen(v, s.a_sbit));
			atomicAdd(bins.counts + bin * bins.copies + copy, 1ull);
		}
	}
}

template <bool V>
__global__ __launch_bounds__(kWorkgroup) void k_bp_scan_pair_gsum(const BpGroup *__restrict__ v_groups,
                                                                  const BpGroup *__restrict__ k_groups,
                                                                  const BpPairArgs s) {
	__shared__ uint4 lds[kBpWaves * 2 * kBpScanWaveChunks];
	__shared__ unsigned long long lds_bins[kBpWaves * 2 * kBpPairBins];
	const BpWaveRun w(s.run, lds, 2);
	if (w.none) return;
	const uint32_t lane = w.lane;
	const uint32_t nbins = s.nkeys + 1u; // <= kBpPairBins
	BpPairBins bins;
	bins.sums = lds_bins + w.wave * 2 * kBpPairBins;
	bins.counts = bins.sums + kBpPairBins;
	bins.copies = nbins <= 16u ? 16u : nbins <= 32u ? 8u : nbins <= 64u ? 4u : nbins <= 128u ? 2u : 1u; // * nbins <= 257
	for (uint32_t i = lane; i < 2 * kBpPairBins; i += 64u) bins.sums[i] = 0ull;
	__builtin_amdgcn_wave_barrier();
	for (uint32_t gi = w.g0; gi < w.g1; gi++) {
		const BpGroup gv = v_groups[gi], gk = k_groups[gi];
		BpCursor cv, ck;
		const int kv = bp_cursor_open(cv, gv, s.a_blocks, s.a_tmask, w.stage);
		const int kk = bp_cursor_open(ck, gk, s.b_blocks, s.b_tmask, w.stage + kBpScanWaveChunks);
		const uint64_t win = bp_group_window<V>(gv, s.validity, lane);
		bp_with_kind(kv, [&](auto tv) __attribute__((always_inline)) {
			bp_with_kind(kk, [&](auto tk) __attribute__((always_inline)) {
				bp_pair_gsum_steps<decltype(tv)::value, decltype(tk)::value>(s, cv, ck, win, lane, bins);
			});
		});
	}
	// the wave's LDS adds have executed before these reads (in order); one global atomic per bin
	__builtin_amdgcn_wave_barrier();
	for (uint32_t b = lane; b < nbins; b += 64u) {
		uint64_t sum = 0ull, cnt = 0ull;
		for (uint32_t c = 0; c < bins.copies; c++) {
			sum += bins.sums[b * bins.copies + c];
			cnt += bins.counts[b * bins.copies + c];
		}
		if (cnt != 0ull) {
			atomicAdd(s.res + b, (unsigned long long)sum);
			if (s.counts != nullptr) atomicAdd(s.counts + b, (unsigned long long)cnt);
		}
	}
}

// ---- select / count the rows where value(a) <cmp> value(b) ----------------------------------------------------

enum : uint32_t { kBpCmpLt = 1u, kBpCmpEq = 2u, kBpCmpGt = 4u }; // ADAC_CMP_* of adacodec.h

struct BpPairCmpArgs {
	BpPairArgs p;               // p.res: rows selected per segment of the first layout
	unsigned long long *bitmap; // select: bit e = element out_off + row of the first layout; nullptr: count only
	uint32_t cmp;               // an OR of kBpCmpLt / Eq / Gt, 1 ... 6
};

// A mathematical integer in [-2^63, 2^64), what a value of any of the eight types is, as the 65-bit number
// value + 2^63 = top * 2^64 + low.  From the value widened to 64 bits by its type's signedness: adding 2^63 flips
// bit 63, and only an unsigned type (sbit = 0, of 64 bits) has values of 2^63 and more.
struct BpMath {
	uint64_t low;
	uint32_t top;
	__device__ __forceinline__ BpMath(uint64_t wide, uint64_t sbit)
	    : low(wide ^ (1ull << 63)), top(sbit == 0ull ? (uint32_t)(wide >> 63) : 0u) {}
};
// the borrow of the 65-bit difference
__device__ __forceinline__ bool bp_math_lt(const BpMath &x, const BpMath &y) {
	return (int32_t)(x.top - y.top - (uint32_t)(x.low < y.low)) < 0;
}
__device__ __forceinline__ bool bp_math_eq(const BpMath &x, const BpMath &y) {
	return ((x.low ^ y.low) | (uint64_t)(x.top ^ y.top)) == 0ull;
}
// which of the three bits of cmp the pair (x, y) answers to
__device__ __forceinline__ uint32_t bp_math_cmp(const BpMath &x, const BpMath &y) {
	return bp_math_lt(x, y) ? kBpCmpLt : bp_math_eq(x, y) ? kBpCmpEq : kBpCmpGt;
}

// A wave-uniform value kept in a vector register from here on: the step loops are short of scalar registers (two
// cursors, the window and the kernel's arguments), and what is needed only at a group's end can wait in a lane.
template <typename T>
__device__ __forceinline__ T bp_park(T x) {
	asm volatile("" : "+v"(x));
	return x;
}
// ... and a parked pointer back in scalar registers for the stretch that reads through it
template <typename T>
__device__ __forceinline__ T *bp_unpark(T *p) {
	const uint64_t v = reinterpret_cast<uint64_t>(p);
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
	const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
	return reinterpret_cast<T *>(((uint64_t)hi << 32) | lo);
}

// [olo, ohi]: the ordered numbers every value of the group lies between, had from the header alone — a constant
// (linear with step 0), or a FOR group whose [frame, frame + 2^w) does not wrap in its type's ordered domain
// (bp_scan_group's test).  false: the group has to be walked.
__device__ __forceinline__ bool bp_cursor_interval(const BpCursor &c, int kind, uint64_t sbit, uint64_t &olo,
                                                   uint64_t &ohi) {
	olo = ohi = (c.frame & c.tmask) ^ sbit;
	if (kind == kBpCurLinear) return c.base == 0ull;
	if (kind != kBpCurFor) return false;
	const uint64_t span = mask64(c.w);
	if (span > c.tmask - olo) return false;
	ohi = olo + span;
	return true;
}

// lane k of the result keeps step k's ballot, as bp_scan_row does for kBpScanRange
template <int KA, int KB>
__device__ __forceinline__ uint64_t bp_pair_cmp_steps(const BpPairArgs &s, uint32_t cmp, BpCursor &ca, BpCursor &cb,
                                                      uint64_t win, uint32_t lane) {
	uint64_t hits = 0ull;
	const uint32_t steps = (ca.n + 63u) >> 6;
	for (uint32_t k = 0; k < steps; k++) {
		const uint64_t wk = bp_readlane64(win, k);
		// nothing of the step is wanted: legal to pass over only when no prefix has to advance
		if (KA != kBpCurDelta && KB != kBpCurDelta && wk == 0ull) continue;
		const uint64_t va = bp_cursor_value<KA>(ca, k, lane);
		const uint64_t vb = bp_cursor_value<KB>(cb, k, lane);
		const BpMath ma(bp_widen(va, s.a_sbit), s.a_sbit), mb(bp_widen(vb, s.b_sbit), s.b_sbit);
		const uint64_t ballot = __ballot(((wk >> lane) & 1ull) && (cmp & bp_math_cmp(ma, mb)) != 0u);
		if (lane == k) hits = ballot;
	}
	return hits;
}

template <bool V>
__global__ __launch_bounds__(kWorkgroup) void k_bp_scan_pair_cmp(const BpGroup *__restrict__ a_groups,
                                                                 const BpGroup *__restrict__ b_groups,
                                                                 const uint32_t *__restrict__ group_seg /* of a */,
                                                                 const BpPairCmpArgs c) {
	__shared__ uint4 lds[kBpWaves * 2 * kBpScanWaveChunks];
	const BpPairArgs &s = c.p;
	const BpWaveRun w(s.run, lds, 2);
	if (w.none) return;
	const uint32_t lane = w.lane;
	BpScanAcc<kBpScanRange> acc;
	// Beside k_bp_scan_pair_sum's state the step loops hold the comparison's lane masks; with everything below in
	// scalar registers the kernel is 4 (<V>: 11) of them short, so what a group needs only at its start or end is parked
	// (the results, the comparison and the mask are read per lane anyway and stay where they are)
	unsigned long long *const res = bp_park(s.res), *const bitmap = bp_park(c.bitmap);
	const uint32_t cmp = bp_park(c.cmp);
	const uint64_t *const validity = bp_park(s.validity);
	const uint8_t *const pa_blocks = bp_park(s.a_blocks), *const pb_blocks = bp_park(s.b_blocks);
	const uint32_t *const pgroup_seg = bp_park(group_seg);
	uint32_t seg = group_seg[w.g0];
	for (uint32_t gi = w.g0; gi < w.g1; gi++) {
		acc.enter(bp_unpark(pgroup_seg)[gi], seg, res, lane);
		const BpGroup ga = a_groups[gi];
		const uint64_t out_off = bp_park(ga.out_off);
		const uint64_t win = bp_group_window<V>(ga, validity, lane);
		// no row of the group is wanted: nothing is read and, the cursors being opened per group, no prefix is owed
		if (V && __ballot(win != 0ull) == 0ull) continue;
		const BpGroup gb = b_groups[gi];
		BpCursor ca, cb;
		const int ka = bp_cursor_open(ca, ga, bp_unpark(pa_blocks), s.a_tmask, w.stage);
		const int kb = bp_cursor_open(cb, gb, bp_unpark(pb_blocks), s.b_tmask, w.stage + kBpScanWaveChunks);
		// the two headers decide the group when every value of a lies on one side of every value of b, or both columns
		// are one value: no payload byte of either is read
		uint32_t is = 0u;
		uint64_t alo, ahi, blo, bhi;
		if (bp_cursor_interval(ca, ka, s.a_sbit, alo, ahi) && bp_cursor_interval(cb, kb, s.b_sbit, blo, bhi)) {
			// (an ordered number less its type's sign bit is the widened value)
			if (bp_math_lt(BpMath(ahi - s.a_sbit, s.a_sbit), BpMath(blo - s.b_sbit, s.b_sbit))) is = kBpCmpLt;
			else if (bp_math_lt(BpMath(bhi - s.b_sbit, s.b_sbit), BpMath(alo - s.a_sbit, s.a_sbit))) is = kBpCmpGt;
			else if (alo == ahi && blo == bhi) is = kBpCmpEq; // neither below the other
		}
		uint64_t hits = 0ull;
		if (is != 0u) {
			hits = (cmp & is) != 0u ? win : 0ull;
		} else {
			bp_with_kind(ka, [&](auto ta) __attribute__((always_inline)) {
				bp_with_kind(kb, [&](auto tb) __attribute__((always_inline)) {
					hits = bp_pair_cmp_steps<decltype(ta)::value, decltype(tb)::value>(s, cmp, ca, cb, win, lane);
				});
			});
		}
		acc.a += (uint64_t)__popcll(hits);
		if (bitmap != nullptr) bp_group_emit(out_off, ga.rows, hits, bitmap, lane);
	}
	acc.flush(res, seg, lane);
}
