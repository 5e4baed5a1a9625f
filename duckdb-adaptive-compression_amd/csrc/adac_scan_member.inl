// adac_scan_member.inl — a filter that tests a row's value against a BIT SET INDEXED BY VALUE, and its counterpart that
// builds such a set from the wanted rows of a packed column: an IN list (TPC-H Q12's l_shipmode IN ('MAIL', 'SHIP')) and
// the two sides of a semi-join on a dense integer key (Q4's EXISTS: build over l_orderkey, probe over o_orderkey),
// nothing decoded to memory.  Included into adac_kernels.hip inside namespace adac::{anonymous}, after
// adac_scan_compare.inl: the kernels have k_scan_compare's shell (one workgroup per ScanGroup, SelOut / sel_or /
// sel_write_out in the plain form, one atomicAdd per wave for the count; the host clears the counts, the bitmap and, for
// the build, d_set).
//
// The set covers the values [set_base, set_base + set_bits - 1] in T's own order; bit i of the 64-bit word i / 64 (bit
// i & 31 of the 32-bit word i / 32) stands for set_base + i.  The index of a value is RangePred's t for lo = set_base,
//   t = (bits(v) ^ sbit) - (bits(set_base) ^ sbit)   in 64-bit unsigned arithmetic,
// and the value is in the domain iff t < set_bits (the host has checked that the domain stays inside the type, so a
// value below the base cannot wrap into it).
//
// A scan group is handled by one READER and one SET ACCESS, both chosen uniformly from the descriptor, the type and
// (set_base, set_bits) alone (member_plan; forms.member_form_groups is its host mirror):
//   header   the segment has a frame (product_frame) and [frame, frame + 2^w - 1] does not meet the domain: no row can
//            be a member.  No packed word and no set word is read; the probe leaves the image zero, the build does
//            nothing.  The zonemap skip of a join filter.
//   walk     frame, 4 <= w <= 32, count * w < 2^31: the width-templated register walk, one wave per RwQuarter
//            (compare_walk without the second column).  Per row one add, t = field + (frame - set_base), the domain
//            test and the set look-up.
//   staged   everything else (widths 1..3 and 33..64, raw signed slots, ADAC_NO_MIN, unpacked segments, frames that
//            wrap): the whole workgroup, the group in stages of packed bytes in LDS, value widened as in
//            compare_generic, t as defined above, the hits of 64 consecutive rows gathered by one ballot per wave.
//   slice    the segment has a frame and the set bits its interval can reach, [lo, hi), are at most kMemberSliceBits:
//            the workgroup copies the 32-bit words of d_set from s0 = lo rounded down to 32 on into LDS (tail bits
//            >= set_bits masked off) and looks rows up there; the build ORs into a zeroed window and afterwards sends
//            its non-zero words to d_set with atomicOr.  Every segment with w <= 16 qualifies.
//   direct   otherwise: the probe loads the word t >> 5 of d_set only when t < set_bits (no out-of-range index is
//            formed), the build does one global atomicOr per hit row.
//
// Barriers: one after the image is zeroed and the window filled, one before image and window are written out; the
// staged reader has two per stage.  EVERY wave reaches every barrier in every form: the reader is chosen uniformly per
// workgroup, a wave whose quarter is empty, and the header form, skip only the walk.

constexpr uint32_t kMemberSliceBits = 65536;
constexpr uint32_t kMemberSliceWords = kMemberSliceBits / 32 + 1;       // [s0, hi) from any bit phase of lo
constexpr uint32_t kMemberSliceChunks = (kMemberSliceWords + 3) / 4;
constexpr uint32_t kMemberStageChunks = 126;                            // ONE stage buffer (the slice takes the rest)
constexpr uint32_t kMemberStageBits = (kMemberStageChunks - 2) * 128u - 256u; // row bits of a stage, from any bit offset
constexpr uint32_t kMemberLdsChunks = kMemberSliceChunks + kMemberStageChunks;
static_assert(kMemberStageBits / 64u >= 64u, "a stage holds 64 rows of 64 bits");
static_assert(kMemberStageChunks <= (uint32_t)kWorkgroup, "a thread stages one chunk");
static_assert(kMemberLdsChunks * 16u + kSelImageWords * 4u <= 18u * 1024u,
              "slice + stage + selection image: eight workgroups per CU");

enum : uint32_t { kMemHeader = 0u, kMemWalk = 1u, kMemStaged = 2u };

struct MemberDomain {
	uint64_t tmask, sbit; // the column type: its all-ones mask and its sign bit (0 for unsigned types)
	uint64_t bbase;       // bits(set_base) ^ sbit
	uint64_t set_bits;    // 1 ... 2^32, bbase + set_bits - 1 <= tmask
};

struct MemberPlan {
	uint32_t reader;
	bool slice;
	uint64_t delta; // walk: (frame ^ sbit) - bbase, so that t = field + delta
	uint64_t s0;    // slice: the set bit of bit 0 of the window, a multiple of 32
	uint32_t nw;    // slice: 32-bit words of the window, 1 ... kMemberSliceWords
};

// Uniform; depends on the descriptor, the type and the domain only.
__device__ __forceinline__ MemberPlan member_plan(const adac_segment_desc &d, const MemberDomain &dom) {
	MemberPlan p {kMemStaged, false, 0ull, 0ull, 0u};
	uint64_t add = 0;
	if (!product_frame(d, dom.tmask, dom.sbit, add)) return p;
	// biased by the sign bit every interval is one of unsigned numbers below 2^64; neither end wraps
	const uint64_t bmin = add + dom.sbit, btop = bmin + mask64(d.width);
	const uint64_t dlo = dom.bbase, dhi = dom.bbase + (dom.set_bits - 1ull);
	if (btop < dlo || dhi < bmin) {
		p.reader = kMemHeader;
		return p;
	}
	const uint64_t lo = bmin > dlo ? bmin - dlo : 0ull;         // set bits [lo, hi) are what the segment can reach
	const uint64_t hi = (btop < dhi ? btop : dhi) - dlo + 1ull; // <= set_bits
	p.slice = hi - lo <= (uint64_t)kMemberSliceBits;
	p.s0 = lo & ~31ull;
	p.nw = p.slice ? (uint32_t)((hi - p.s0 + 31ull) >> 5) : 0u;
	p.delta = bmin - dlo;
	if (d.width >= 4u && d.width <= 32u && (uint64_t)d.count * d.width < (1ull << 31)) p.reader = kMemWalk;
	return p;
}

// The look-up and the OR, for both readers.  slice form: every row of the group whose t is in the domain has
// s0 <= t < s0 + 32 * nw (its field has w bits, whatever the row holds).
struct MemberSet {
	uint32_t *slice; // the LDS window
	uint32_t *set32; // d_set as 32-bit words
	uint64_t s0, set_bits;
	bool in_slice;   // uniform
	// probe: is t a member?  build: if the row is wanted and t in the domain, set its bit; returns whether it was
	template <bool BUILD>
	__device__ __forceinline__ bool touch(uint64_t t, bool want) const {
		const bool in = t < set_bits;
		if (in_slice) {
			const uint32_t r = in ? (uint32_t)(t - s0) : 0u;
			if (BUILD) {
				if (in && want) atomicOr(&slice[r >> 5], 1u << (r & 31u));
				return in && want;
			}
			return in && ((slice[r >> 5] >> (r & 31u)) & 1u) != 0u;
		}
		if (BUILD) {
			if (in && want) atomicOr(set32 + (t >> 5), 1u << ((uint32_t)t & 31u));
			return in && want;
		}
		uint32_t wv = 0u;
		if (in && want) wv = set32[t >> 5];
		return ((wv >> ((uint32_t)t & 31u)) & 1u) != 0u;
	}
};

// d_set -> the window (probe; words past the set's end are zero, the tail bits >= set_bits masked off), or a zeroed
// window (build).  The whole workgroup; the caller's barrier follows.
template <bool BUILD>
__device__ __forceinline__ void member_slice_fill(const MemberPlan &plan, const MemberSet &set) {
	const uint64_t n32 = ((set.set_bits + 63ull) >> 6) * 2ull; // 32-bit words of d_set
	for (uint32_t i = threadIdx.x; i < plan.nw; i += (uint32_t)kWorkgroup) {
		uint32_t v = 0u;
		if (!BUILD) {
			const uint64_t gw = (plan.s0 >> 5) + i;
			v = set.set32[gw < n32 ? gw : n32 - 1ull]; // unconditional, index clamped into the set
			const uint64_t bit0 = gw << 5;
			if (gw >= n32 || bit0 >= set.set_bits) v = 0u;
			else if (set.set_bits - bit0 < 32ull) v &= (1u << (uint32_t)(set.set_bits - bit0)) - 1u;
		}
		set.slice[i] = v;
	}
}

// build, after the barrier: the window's non-zero words -> d_set
__device__ __forceinline__ void member_slice_flush(const MemberPlan &plan, const MemberSet &set) {
	for (uint32_t i = threadIdx.x; i < plan.nw; i += (uint32_t)kWorkgroup) {
		const uint32_t v = set.slice[i];
		if (v) atomicOr(set.set32 + (plan.s0 >> 5) + i, v);
	}
}

// Reader "walk": rows [r0, r1) of the segment, walked by ONE wave (compare_walk without the second column).  `count`
// gains the lane's hits, the image their bits.
template <int W, bool V, bool SEL, bool BUILD>
__device__ __forceinline__ void member_walk(uint32_t r0, uint32_t r1, const adac_segment_desc &d,
                                            const uint4 *__restrict__ seg16, const uint64_t *__restrict__ validity,
                                            uint64_t delta, const MemberSet &set, const SelOut &sel_out,
                                            uint32_t &count) {
	constexpr int MAXV = ChunkWindow<W>::MAXV;
	const ChunkRange<W> run(r0, r1, d.count);
	const uint32_t c0 = run.c0, c1 = run.c1;
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t sh0 = (uint32_t)(d.val_off & 31u);
	uint32_t L = c0 + lane;
	uint4 q;
	uint32_t e;
	run.load(seg16, L, q, e);
	const ChunkMask<W, V> vmask(validity, d.val_off, r1);
	uint64_t vm0 = 0, vm1 = 0;
	if (V) vmask.words(run.clamp(L), vm0, vm1);
	for (uint32_t round0 = c0; round0 < c1; round0 += 64u, L += 64u) { // uniform trip count
		uint4 qn;
		uint32_t en;
		run.load(seg16, L + 64u, qn, en);
		uint64_t vn0 = 0, vn1 = 0;
		if (V) vmask.words(run.clamp(L + 64u), vn0, vn1);
		if (L < c1) {
			const ChunkWindow<W> cw(q, e, L, r1);
			const uint32_t have = cw.have();
			// rows that exist AND are wanted, as one mask
			uint32_t vb = have >= 32u ? 0xffffffffu : ((1u << have) - 1u);
			if (V) vb &= (uint32_t)vmask.window(vm0, vm1, cw.i0 < r1 ? cw.i0 : r1);
			uint32_t hits = 0;
#pragma unroll
			for (int j = 0; j < MAXV; j++) {
				const uint64_t t = (uint64_t)field_of<W>(cw.nrm, j) + delta;
				hits |= (set.template touch<BUILD>(t, ((vb >> j) & 1u) != 0u) ? 1u : 0u) << j;
			}
			hits &= vb;
			count += (uint32_t)__popc(hits);
			if (SEL) sel_or(sel_out, sh0 + cw.i0, hits, have);
		}
		q = qn;
		e = en;
		vm0 = vn0;
		vm1 = vn1;
	}
}

// Reader "staged": the whole workgroup, the group in stages (compare_generic's structure for one column, one buffer:
// the next stage's chunks are loaded while this one is consumed and stored between two barriers).  Every thread runs
// every barrier.  Lane 0 of each wave counts the wave's hits.
template <bool V, bool SEL, bool BUILD>
__device__ __forceinline__ uint32_t member_staged(const ScanGroup &g, const uint64_t *__restrict__ words,
                                                  const MemberDomain &dom, const uint64_t *__restrict__ validity,
                                                  uint4 *stage, const MemberSet &set, const SelOut &sel_out) {
	const adac_segment_desc &d = g.d;
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const uint32_t w = d.width;
	const uint32_t per_stage = (kMemberStageBits / w) & ~63u; // >= 64 rows
	const uint4 *s16 = reinterpret_cast<const uint4 *>(words + d.word_off);
	const uint64_t add = effective_add(d);
	const uint32_t sh0 = (uint32_t)(d.val_off & 31u);
	const uint32_t mlo = w >= 32u ? 0xffffffffu : mask32(w), mhi = w > 32u ? mask32(w - 32u) : 0u;
	const uint32_t *s32 = reinterpret_cast<const uint32_t *>(stage);
	struct Stage {
		const uint4 *src; // the 16-byte chunk holding the first bit of the rows
		uint32_t bit0, chunks, row0, m;
	};
	auto make_stage = [&](uint32_t done, Stage &st) -> bool {
		if (done >= g.n) return false;
		st.row0 = g.first + done;
		st.m = g.n - done < per_stage ? g.n - done : per_stage;
		const uint64_t pos = (uint64_t)st.row0 * w;
		st.src = s16 + (pos >> 7);
		st.bit0 = (uint32_t)(pos & 127);
		st.chunks = (st.bit0 + st.m * w + 127u) >> 7; // 1 ... kMemberStageChunks - 3
		return true;
	};
	Stage cur, nxt;
	uint32_t done = 0;
	bool have = make_stage(done, cur); // uniform
	uint4 q = make_uint4(0u, 0u, 0u, 0u);
	if (have) q = cur.src[tid < cur.chunks ? tid : cur.chunks - 1u];
	uint32_t count = 0;
	while (have) { // uniform
		if (tid < cur.chunks) stage[tid] = q;
		__syncthreads();
		done += cur.m;
		const bool more = make_stage(done, nxt);
		// in flight while this stage is consumed: an unconditional load, index clamped into the stage
		if (more) q = nxt.src[tid < nxt.chunks ? tid : nxt.chunks - 1u];
		const uint64_t elem0 = d.val_off + cur.row0;
		// a wave takes 64 consecutive rows at a time: uniform trip count, so every lane is there for the ballot
		for (uint32_t base = 0; base < cur.m; base += (uint32_t)kWorkgroup) {
			const uint32_t row = base + tid;
			const uint32_t rr = row < cur.m ? row : cur.m - 1u; // clamped: the reads stay inside the stage and the mask
			const uint64_t f = staged_field(s32, cur.bit0 + rr * w, mlo, mhi);
			const uint32_t keep = V ? (validity_window_pair(validity, elem0 + rr, 1u) & 1u) : 1u;
			const uint64_t t = ((((f + add) & dom.tmask) ^ dom.sbit) - dom.bbase);
			const bool want = row < cur.m && keep != 0u;
			const bool hit = set.template touch<BUILD>(t, want) && want;
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
		__syncthreads(); // every thread has read the stage
		cur = nxt;
		have = more;
	}
	return count;
}

// What the probe and the build kernel share.  V: a mask is given; SEL: a bitmap is written (probe); BUILD: rows set
// bits instead of testing them.
template <bool V, bool SEL, bool BUILD>
__device__ __forceinline__ void member_scan(const ScanGroup *__restrict__ groups, const uint64_t *__restrict__ words,
                                            const MemberDomain &dom, const uint64_t *__restrict__ validity,
                                            uint32_t *set32, uint32_t *__restrict__ bitmap32,
                                            unsigned long long *__restrict__ counts, uint4 *lds, uint32_t *sel_img) {
	const ScanGroup g = load_scan_group(groups, blockIdx.x);
	const MemberPlan plan = member_plan(g.d, dom);
	const MemberSet set {reinterpret_cast<uint32_t *>(lds), set32, plan.s0, dom.set_bits, plan.slice};
	const uint32_t sel_p0 = (uint32_t)(g.d.val_off & 31u) + g.first; // the group's positions [sel_p0, sel_p0 + n)
	SelOut sel_out {sel_img, bitmap32, sel_p0 & ~31u, 0, nullptr, false, nullptr, 0u, 0u, 0u, 0u};
	const bool live = plan.reader != kMemHeader; // uniform
	if (SEL) {
		const uint32_t nwords = (sel_p0 + g.n - sel_out.p_base + 31u) >> 5; // <= kSelMaxRows / 32 + 2
		for (uint32_t i = threadIdx.x; i < nwords; i += kWorkgroup) sel_img[i] = 0u;
	}
	if (live && plan.slice) member_slice_fill<BUILD>(plan, set);
	__syncthreads();
	uint32_t count = 0;
	if (plan.reader == kMemWalk) {
		const RwQuarter qr(g, threadIdx.x >> 6);
		if (!qr.empty()) { // uniform per wave; the walk has no barrier, the ones below are reached by every wave
			dispatch_width_4_32(g.d.width, [&](auto wc) __attribute__((always_inline)) {
				member_walk<decltype(wc)::value, V, SEL, BUILD>(qr.r0, qr.r1, g.d,
				                                                reinterpret_cast<const uint4 *>(words + g.d.word_off),
				                                                validity, plan.delta, set, sel_out, count);
			});
		}
	} else if (plan.reader == kMemStaged) {
		count = member_staged<V, SEL, BUILD>(g, words, dom, validity, lds + kMemberSliceChunks, set, sel_out);
	}
	const uint64_t tot = wave_sum((uint64_t)count);
	if ((threadIdx.x & 63u) == 0u && tot != 0ull) atomicAdd(counts + g.seg, (unsigned long long)tot);
	__syncthreads(); // every wave's bits are in the image / the window
	if (SEL && live) sel_write_out(sel_out, bitmap32 + (g.d.val_off >> 5), sel_p0, sel_p0 + g.n);
	if (BUILD && live && plan.slice) member_slice_flush(plan, set);
}

// Probe.  V: a mask is given; SEL: a bitmap is written.
template <bool V, bool SEL>
__global__ __launch_bounds__(kWorkgroup) void k_scan_member(const ScanGroup *__restrict__ groups,
                                                            const uint64_t *__restrict__ words, MemberDomain dom,
                                                            const uint64_t *__restrict__ validity, uint32_t *set32,
                                                            uint32_t *__restrict__ bitmap32,
                                                            unsigned long long *__restrict__ counts) {
	__shared__ uint4 lds[kMemberLdsChunks];
	__shared__ uint32_t sel_img[SEL ? kSelImageWords : 1];
	member_scan<V, SEL, false>(groups, words, dom, validity, set32, bitmap32, counts, lds, sel_img);
}

// Build.  V: a mask is given.
template <bool V>
__global__ __launch_bounds__(kWorkgroup) void k_scan_member_build(const ScanGroup *__restrict__ groups,
                                                                  const uint64_t *__restrict__ words, MemberDomain dom,
                                                                  const uint64_t *__restrict__ validity, uint32_t *set32,
                                                                  unsigned long long *__restrict__ counts) {
	__shared__ uint4 lds[kMemberLdsChunks];
	__shared__ uint32_t sel_img[1];
	member_scan<V, false, true>(groups, words, dom, validity, set32, nullptr, counts, lds, sel_img);
}
