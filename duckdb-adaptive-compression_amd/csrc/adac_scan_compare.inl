// adac_scan_compare.inl — a filter that looks at TWO packed columns of one table: select / count the rows where
// value(a) <cmp> value(b) (TPC-H Q12's `l_commitdate < l_receiptdate`), nothing decoded to memory.  Included into
// adac_kernels.hip inside namespace adac::{anonymous}, after adac_sum_product.inl: the kernel has k_scan_product's shape
// (one workgroup per ScanGroup of `a`, b's descriptor through load_desc_scalar, RwQuarter, product_frame,
// product_fast_eligible, the clamped chunk loads of product_walk and the stage structure of product_generic), the
// selection image of the filter scan (SelOut, sel_or, sel_write_out) and the 65-bit order of the BITPACKING compare
// (BpMath, adac_bp_pair_scans.inl).
//
// The values compare as mathematical integers, each widened by its own column's signedness; rows whose bit is clear in
// the mask (a's element space) are not selected.  Three forms, chosen per group, uniformly, from the two descriptors
// and the two types alone (compare_plan):
//   header   both columns have a frame (product_frame: value = field + frame without leaving the type), so each
//            column's values lie in [frame, frame + 2^w - 1], and the two intervals are disjoint (or both are single
//            values): every row of the group answers alike.  The hits are the group's mask bits (all of its rows
//            without a mask) when cmp holds the deciding bit, otherwise none.  No packed word of either column is read.
//   fast     product_fast_eligible's conditions and overlapping intervals: product_walk with the arithmetic replaced.
//            With d = frame_b - frame_a (|d| < 2^32, the header form took the rest) a row is decided by
//            t = field_a - field_b against d, and every cmp is ONE range test of t in 64-bit unsigned arithmetic
//            ((t - lo) <= span; NE is EQ inverted): two subtracts and a compare per row, no widening.  A lane's hits of
//            a chunk are one mask of up to 32 consecutive rows.
//   generic  everything else (widths 1..64, raw signed slots, ADAC_NO_MIN, unpacked segments, frames that wrap, the
//            all-ones stored min): product_generic's stages, value = (((field + effective_add) & tmask) ^ sbit) - sbit
//            per column, bp_math_cmp per row, the hits of 64 consecutive rows gathered by one ballot per wave.
// Result: the host clears d_counts and the bitmap; every wave adds its count with one atomicAdd per group, the bitmap
// goes image -> global with sel_write_out in its plain form (stores for the words wholly inside the group, atomicOr for
// the two words a group may share with a neighbour).  No arrival cells, no edge records, not persistent.
//
// Barriers: with SEL the kernel has one after the image is zeroed and one before it is written out.  EVERY wave reaches
// both in every form; a wave whose quarter is empty, and the header form, skip only the walk.

constexpr uint32_t kCmpStageBytes = 2048;                    // generic form: packed bytes of one column per stage
constexpr uint32_t kCmpStageChunks = kCmpStageBytes / 16 + 2; // one stage buffer of one column
constexpr uint32_t kCmpLdsChunks = (kWorkgroup / 64) * kProdWaveChunks;
static_assert(4 * kCmpStageChunks <= kCmpLdsChunks, "the two walked forms share one LDS block");
static_assert(kCmpStageBytes / 16 + 1 <= kWorkgroup, "a thread stages one chunk per column");
static_assert((kCmpStageBytes * 8u - 256u) / 64u < (uint32_t)kWorkgroup && kWorkgroup * 64u / 128u + 1u < kCmpStageChunks,
              "the smallest stage (kWorkgroup rows of 64 bits from any bit offset) fits a buffer");
static_assert(kCmpLdsChunks * 16u + kSelImageWords * 4u <= 18u * 1024u, "stage + selection image: eight workgroups per CU");

enum : uint32_t { kCmpHeader = 0u, kCmpFast = 1u, kCmpGeneric = 2u };

struct ComparePlan {
	uint32_t form;
	uint32_t is;   // header: which of kBpCmpLt / Eq / Gt every row of the group answers to
	int64_t d;     // fast: frame_b - frame_a
};

// Uniform; depends on the two descriptors and the types only.
__device__ __forceinline__ ComparePlan compare_plan(const adac_segment_desc &ad, const adac_segment_desc &bd,
                                                    const ProductTypes &ty) {
	ComparePlan p {kCmpGeneric, 0u, 0};
	uint64_t ma = 0, mb = 0;
	if (!product_frame(ad, ty.a_tmask, ty.a_sbit, ma) || !product_frame(bd, ty.b_tmask, ty.b_sbit, mb)) return p;
	const uint64_t sa = mask64(ad.width), sb = mask64(bd.width); // frame + 2^w - 1 stays inside the type
	const BpMath alo(ma, ty.a_sbit), ahi(ma + sa, ty.a_sbit), blo(mb, ty.b_sbit), bhi(mb + sb, ty.b_sbit);
	if (bp_math_lt(ahi, blo)) {
		p.form = kCmpHeader;
		p.is = kBpCmpLt;
	} else if (bp_math_lt(bhi, alo)) {
		p.form = kCmpHeader;
		p.is = kBpCmpGt;
	} else if (sa == 0ull && sb == 0ull) { // two single values that are not apart
		p.form = kCmpHeader;
		p.is = kBpCmpEq;
	} else if (product_fast_eligible(ad, bd, ty).ok) {
		p.form = kCmpFast;
		p.d = (int64_t)(mb - ma); // the intervals overlap and are at most 2^32 long: the difference mod 2^64 is exact
	}
	return p;
}

// cmp as a range test of t = field_a - field_b (|t| < 2^32) against d (|d| < 2^32): hit = ((t - lo) <= span) != inv
struct CompareRange {
	uint64_t lo, span;
	uint32_t inv; // 0 / ~0
	__device__ __forceinline__ CompareRange(uint32_t cmp, int64_t d) {
		constexpr uint64_t kFar = 1ull << 34; // further than t - d reaches
		const uint32_t c = (cmp == (kBpCmpLt | kBpCmpGt)) ? kBpCmpEq : cmp;
		inv = c != cmp ? ~0u : 0u;
		const uint64_t ud = (uint64_t)d;
		lo = (c & kBpCmpLt) ? ud - kFar : (c & kBpCmpEq) ? ud : ud + 1ull;
		const uint64_t hi = (c & kBpCmpGt) ? ud + kFar : (c & kBpCmpEq) ? ud : ud - 1ull;
		span = hi - lo;
	}
};

// Fast form: rows [r0, r1) of the segment pair, walked by ONE wave (product_walk with the arithmetic replaced).
// Returns nothing; `count` gains the lane's hits, the image their bits.
template <int W, bool V, bool SEL>
__device__ __forceinline__ void compare_walk(uint32_t r0, uint32_t r1, const adac_segment_desc &ad,
                                             const adac_segment_desc &bd, const uint4 *__restrict__ aseg16,
                                             const uint4 *__restrict__ bseg16, const uint64_t *__restrict__ validity,
                                             uint4 *bstage, const CompareRange &cr, const SelOut &sel_out,
                                             uint32_t &count) {
	constexpr int MAXV = ChunkWindow<W>::MAXV;
	const uint32_t wb = bd.width, bmask = mask32(wb);
	// as many lanes as keep the round's rows of b inside the buffer (product_walk's bound)
	uint32_t lanes = ((kProdWaveData - 2u) * 128u) / ((uint32_t)MAXV * wb);
	lanes = lanes < 64u ? lanes : 64u;
	const ChunkRange<W> run(r0, r1, ad.count);
	const uint32_t c0 = run.c0, c1 = run.c1;
	const uint32_t bclast = (uint32_t)(((uint64_t)bd.count * wb + 127) >> 7) - 1; // last chunk holding data bits of b
	const uint32_t lane = threadIdx.x & 63u;
	const bool walker = lane < lanes;
	const uint32_t sh0 = (uint32_t)(ad.val_off & 31u);
	uint32_t L = c0 + lane;
	uint4 q;
	uint32_t e;
	run.load(aseg16, L, q, e);
	const ChunkMask<W, V> vmask(validity, ad.val_off, r1); // a's element space
	uint64_t vm0 = 0, vm1 = 0;
	if (V) vmask.words(run.clamp(L), vm0, vm1);
	auto round_b = [&](uint32_t rc, uint32_t &bc0, uint32_t &nb) {
		const uint32_t lo = chunk_first_row<W>(rc);
		uint32_t hi = chunk_first_row<W>(rc + lanes);
		hi = hi < r1 ? hi : r1;
		bc0 = (lo * wb) >> 7;
		nb = hi > lo ? ((hi * wb + 127u) >> 7) - bc0 : 0u;
	};
	auto load_b = [&](uint32_t bc0, uint4 (&bq)[2]) { // unconditional, index clamped into the segment
#pragma unroll
		for (uint32_t p = 0; p < 2; p++) {
			const uint32_t c = bc0 + lane + 64u * p;
			bq[p] = bseg16[c < bclast ? c : bclast];
		}
	};
	auto store_b = [&](const uint4 (&bq)[2], uint32_t nb) {
#pragma unroll
		for (uint32_t p = 0; p < 2; p++) {
			if (lane + 64u * p < nb) bstage[lane + 64u * p] = bq[p];
		}
	};
	const uint32_t *b32 = reinterpret_cast<const uint32_t *>(bstage);
	uint32_t bc0 = 0, nb = 0;
	uint4 bq[2];
	round_b(c0, bc0, nb);
	load_b(bc0, bq);
	store_b(bq, nb);
	for (uint32_t round0 = c0; round0 < c1; round0 += lanes, L += lanes) { // uniform trip count
		uint4 qn;
		uint32_t en;
		run.load(aseg16, L + lanes, qn, en);
		uint64_t vn0 = 0, vn1 = 0;
		if (V) vmask.words(run.clamp(L + lanes), vn0, vn1);
		uint32_t bc0n = 0, nbn = 0;
		round_b(round0 + lanes, bc0n, nbn);
		load_b(bc0n, bq);
		if (walker && L < c1) {
			const ChunkWindow<W> cw(q, e, L, r1);
			const uint32_t have = cw.have();
			// rows that exist AND are wanted, as one mask
			uint32_t vb = have >= 32u ? 0xffffffffu : ((1u << have) - 1u);
			if (V) vb &= (uint32_t)vmask.window(vm0, vm1, cw.i0 < r1 ? cw.i0 : r1);
			const uint32_t bbit = cw.i0 * wb - 128u * bc0; // row i0 of b inside the staged chunks
			uint32_t hits = 0;
#pragma unroll
			for (int j0 = 0; j0 < MAXV; j0 += 8) {
				uint32_t fb[8];
#pragma unroll
				for (int u = 0; u < 8; u++) {
					if (j0 + u < MAXV) fb[u] = staged_field32(b32, bbit + (uint32_t)(j0 + u) * wb, bmask);
				}
#pragma unroll
				for (int u = 0; u < 8; u++) {
					if (j0 + u < MAXV) {
						const uint64_t t = (uint64_t)field_of<W>(cw.nrm, j0 + u) - (uint64_t)fb[u];
						hits |= ((t - cr.lo) <= cr.span ? 1u : 0u) << (j0 + u);
					}
				}
			}
			hits = (hits ^ cr.inv) & vb;
			count += (uint32_t)__popc(hits);
			if (SEL) sel_or(sel_out, sh0 + cw.i0, hits, have);
		}
		q = qn;
		e = en;
		vm0 = vn0;
		vm1 = vn1;
		store_b(bq, nbn); // after this round's reads of the buffer
		bc0 = bc0n;
	}
}

// one stage of the generic form: rows [row0, row0 + m) of the segment pair (all uniform)
struct CompareStage {
	const uint4 *asrc, *bsrc; // the 16-byte chunks holding the first bit of the rows
	uint32_t abit0, bbit0, achunks, bchunks, row0, m;
};

// Generic form: the whole workgroup, the group in stages (product_generic's structure).  Every thread runs every
// barrier.  Lane 0 of each wave counts the wave's hits.
template <bool V, bool SEL>
__device__ __forceinline__ uint32_t compare_generic(const ScanGroup &g, const adac_segment_desc &bd,
                                                    const uint64_t *__restrict__ awords,
                                                    const uint64_t *__restrict__ bwords, const ProductTypes &ty,
                                                    const uint64_t *__restrict__ validity, uint32_t cmp, uint4 *lds,
                                                    const SelOut &sel_out) {
	uint4 *astage[2] = {lds, lds + kCmpStageChunks};
	uint4 *bstage[2] = {lds + 2 * kCmpStageChunks, lds + 3 * kCmpStageChunks};
	const adac_segment_desc &ad = g.d;
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const uint32_t wa = ad.width, wb = bd.width;
	const uint32_t wmax = wa > wb ? wa : wb;
	uint32_t per_stage = ((kCmpStageBytes * 8u - 256u) / wmax) & ~(uint32_t)(kWorkgroup - 1);
	per_stage = per_stage < (uint32_t)kWorkgroup ? (uint32_t)kWorkgroup : per_stage;
	const uint4 *a16 = reinterpret_cast<const uint4 *>(awords + ad.word_off);
	const uint4 *b16 = reinterpret_cast<const uint4 *>(bwords + bd.word_off);
	const uint64_t aadd = effective_add(ad), badd = effective_add(bd);
	const uint32_t sh0 = (uint32_t)(ad.val_off & 31u);
	auto make_stage = [&](uint32_t done, CompareStage &st) -> bool {
		if (done >= g.n) return false;
		st.row0 = g.first + done;
		st.m = g.n - done < per_stage ? g.n - done : per_stage;
		const uint64_t apos = (uint64_t)st.row0 * wa, bpos = (uint64_t)st.row0 * wb;
		st.asrc = a16 + (apos >> 7);
		st.bsrc = b16 + (bpos >> 7);
		st.abit0 = (uint32_t)(apos & 127);
		st.bbit0 = (uint32_t)(bpos & 127);
		st.achunks = (st.abit0 + st.m * wa + 127u) >> 7; // <= kCmpStageBytes / 16 + 1: one per thread, >= 1
		st.bchunks = (st.bbit0 + st.m * wb + 127u) >> 7;
		return true;
	};
	CompareStage cur, nxt;
	uint32_t done = 0;
	bool have = make_stage(done, cur); // uniform
	uint4 aq, bq;
	if (have) {
		if (tid < cur.achunks) astage[0][tid] = cur.asrc[tid];
		if (tid < cur.bchunks) bstage[0][tid] = cur.bsrc[tid];
	}
	__syncthreads();
	const uint32_t amlo = wa >= 32u ? 0xffffffffu : mask32(wa), amhi = wa > 32u ? mask32(wa - 32u) : 0u;
	const uint32_t bmlo = wb >= 32u ? 0xffffffffu : mask32(wb), bmhi = wb > 32u ? mask32(wb - 32u) : 0u;
	uint32_t count = 0;
	uint32_t buf = 0;
	while (have) { // uniform
		done += cur.m;
		const bool more = make_stage(done, nxt);
		if (more) { // in flight while this stage is consumed: unconditional loads, index clamped into the stage
			aq = nxt.asrc[tid < nxt.achunks ? tid : nxt.achunks - 1u];
			bq = nxt.bsrc[tid < nxt.bchunks ? tid : nxt.bchunks - 1u];
		}
		const uint32_t *a32 = reinterpret_cast<const uint32_t *>(astage[buf]);
		const uint32_t *b32 = reinterpret_cast<const uint32_t *>(bstage[buf]);
		const uint64_t elem0 = ad.val_off + cur.row0; // a's element space
		// a wave takes 64 consecutive rows at a time: uniform trip count, so every lane is there for the ballot
		for (uint32_t base = 0; base < cur.m; base += (uint32_t)kWorkgroup) {
			const uint32_t row = base + tid;
			const uint32_t rr = row < cur.m ? row : cur.m - 1u; // clamped: the reads stay inside the stage and the mask
			const uint64_t fa = staged_field(a32, cur.abit0 + rr * wa, amlo, amhi);
			const uint64_t fb = staged_field(b32, cur.bbit0 + rr * wb, bmlo, bmhi);
			const uint32_t keep = V ? (validity_window_pair(validity, elem0 + rr, 1u) & 1u) : 1u;
			uint64_t x = (fa + aadd) & ty.a_tmask;
			x = (x ^ ty.a_sbit) - ty.a_sbit; // widened by a's signedness
			uint64_t y = (fb + badd) & ty.b_tmask;
			y = (y ^ ty.b_sbit) - ty.b_sbit;
			const bool hit = row < cur.m && keep && (cmp & bp_math_cmp(BpMath(x, ty.a_sbit), BpMath(y, ty.b_sbit))) != 0u;
			const uint64_t ballot = __ballot(hit); // rows cur.row0 + base + 64 * wave + [0, 64)
			if (lane == 0u) {
				count += (uint32_t)__popcll(ballot);
				if (SEL) {
					const uint32_t p = sh0 + cur.row0 + base + (tid & ~63u);
					sel_or(sel_out, p, (uint32_t)ballot, 32u);
					sel_or(sel_out, p + 32u, (uint32_t)(ballot >> 32), 32u);
				}
			}
		}
		if (more) {
			if (tid < nxt.achunks) astage[buf ^ 1u][tid] = aq;
			if (tid < nxt.bchunks) bstage[buf ^ 1u][tid] = bq;
		}
		__syncthreads();
		cur = nxt;
		have = more;
		buf ^= 1u;
	}
	return count;
}

// Header form: every row of the group answers alike; the hits are the group's wanted rows (all != 0) or none.  The
// whole workgroup, 32 rows per thread and step; only mask words are read.
template <bool V, bool SEL>
__device__ __forceinline__ uint32_t compare_header(const ScanGroup &g, bool all, const uint64_t *__restrict__ validity,
                                                   const SelOut &sel_out) {
	uint32_t count = 0;
	if (!all) return count; // uniform: the image stays zero
	const uint32_t sh0 = (uint32_t)(g.d.val_off & 31u);
	for (uint32_t at = 32u * threadIdx.x; at < g.n; at += 32u * (uint32_t)kWorkgroup) {
		const uint32_t n = g.n - at < 32u ? g.n - at : 32u;
		uint32_t bits = n >= 32u ? 0xffffffffu : ((1u << n) - 1u);
		if (V) bits &= validity_window_pair(validity, g.d.val_off + g.first + at, n);
		count += (uint32_t)__popc(bits);
		if (SEL) sel_or(sel_out, sh0 + g.first + at, bits, n);
	}
	return count;
}

// V: a mask is given; SEL: a bitmap is written.
template <bool V, bool SEL>
__global__ __launch_bounds__(kWorkgroup) void k_scan_compare(const ScanGroup *__restrict__ agroups,
                                                             const uint64_t *__restrict__ awords,
                                                             const adac_segment_desc *__restrict__ bdescs,
                                                             const uint64_t *__restrict__ bwords, ProductTypes ty,
                                                             const uint64_t *__restrict__ validity, uint32_t cmp,
                                                             uint32_t *__restrict__ bitmap32,
                                                             unsigned long long *__restrict__ counts) {
	__shared__ uint4 lds[kCmpLdsChunks];
	__shared__ uint32_t sel_img[SEL ? kSelImageWords : 1];
	const ScanGroup g = load_scan_group(agroups, blockIdx.x);
	const adac_segment_desc bd = load_desc_scalar(bdescs, g.seg);
	const ComparePlan plan = compare_plan(g.d, bd, ty);
	const uint32_t sel_p0 = (uint32_t)(g.d.val_off & 31u) + g.first; // the group's positions [sel_p0, sel_p0 + n)
	SelOut sel_out {sel_img, bitmap32, sel_p0 & ~31u, 0, nullptr, false, nullptr, 0u, 0u, 0u, 0u};
	if (SEL) {
		const uint32_t nwords = (sel_p0 + g.n - sel_out.p_base + 31u) >> 5; // <= kSelMaxRows / 32 + 2
		for (uint32_t i = threadIdx.x; i < nwords; i += kWorkgroup) sel_img[i] = 0u;
		__syncthreads();
	}
	uint32_t count = 0;
	if (plan.form == kCmpHeader) { // uniform
		count = compare_header<V, SEL>(g, (cmp & plan.is) != 0u, validity, sel_out);
	} else if (plan.form == kCmpFast) {
		const uint32_t wave = threadIdx.x >> 6;
		const RwQuarter qr(g, wave);
		if (!qr.empty()) { // uniform per wave; the walk has no barrier, the ones below are reached by every wave
			const CompareRange cr(cmp, plan.d);
			dispatch_width_4_32(g.d.width, [&](auto wc) __attribute__((always_inline)) {
				compare_walk<decltype(wc)::value, V, SEL>(qr.r0, qr.r1, g.d, bd,
				                                          reinterpret_cast<const uint4 *>(awords + g.d.word_off),
				                                          reinterpret_cast<const uint4 *>(bwords + bd.word_off), validity,
				                                          lds + wave * kProdWaveChunks, cr, sel_out, count);
			});
		}
	} else {
		count = compare_generic<V, SEL>(g, bd, awords, bwords, ty, validity, cmp, lds, sel_out);
	}
	const uint64_t tot = wave_sum((uint64_t)count);
	if ((threadIdx.x & 63u) == 0u && tot != 0ull) atomicAdd(counts + g.seg, (unsigned long long)tot);
	if (SEL) {
		__syncthreads(); // every wave's bits are in the image
		// (a header group without hits has nothing to add to the cleared bitmap; uniform)
		if (plan.form != kCmpHeader || (cmp & plan.is) != 0u) {
			sel_write_out(sel_out, bitmap32 + (g.d.val_off >> 5), sel_p0, sel_p0 + g.n);
		}
	}
}
