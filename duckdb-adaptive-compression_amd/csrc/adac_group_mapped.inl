// adac_group_mapped.inl — SUM(value), COUNT(*) GROUP BY A CODE LOOKED UP THROUGH A DENSE KEY over two packed columns of
// one table (TPC-H Q5's revenue per nation of the supplier behind l_suppkey, Q10 / Q3 through o_custkey / l_orderkey,
// Q14 / Q19 through l_partkey), and the scan that builds such a map from a dimension table with sparse keys.  Nothing is
// decoded to memory, there is no hash table and no global atomic per row.  Included into adac_kernels.hip inside
// namespace adac::{anonymous}, after adac_group_dense.inl: the kernels have k_group_dense's shell (one workgroup per
// ScanGroup of the KEY layout, the host clears the outputs, one atomicAdd per wave for the rows per segment, not
// persistent), its domain (MemberDomain) and its readers (dense_plan: header / walk / staged, the value column's
// eligibility for the walk included).  The walk and the two staged readers are written again here over a SINK (what a
// wanted row inside the domain does with its index t and its value v) rather than factored out of dense_walk: the four
// k_group_dense kernels stay byte for byte what they were.
//
// The map holds one byte per index of the domain, in an allocation of key_span rounded up to a multiple of 8 bytes.
//   slice    the key segment has a frame and the indices its interval can reach, [lo, hi), are at most kMappedSlice:
//            the workgroup copies the 64-bit words of d_map from s0 = lo rounded down to 8 on into LDS (word index
//            clamped into the allocation, as member_slice_fill does) and looks rows up there.  Every key segment of
//            w <= 11, and every domain of at most 2 048 keys (nations, regions, a year of dates), takes the slice.
//   direct   otherwise: a predicated byte load of d_map + t only for a wanted row with t < key_span.  No out-of-range
//            address is formed.
//
// The probe's bins: a row of group g < ngroups adds into one of `copies` copies of the ngroups LDS bins (64-bit sums,
// 32-bit counts: a scan group's rows fit), the copy chosen by lane id; rows with g >= ngroups (the overflow entry, where
// a filtered join sends most rows) add into the lane's registers and leave through one wave reduction.  After the last
// barrier thread g adds up the copies of bin g and sends a non-zero total out with ONE global atomicAdd per output array.
// Integer sums mod 2^64 commute, so the results depend neither on the number of copies nor on the order of arrival.
//
// The build stores min(code, 255) with a plain byte store to d_map + t; the host has filled the map, pad included.
//
// Barriers: one after the bins are zeroed and the slice is filled, one before the bins are written out; the staged
// readers have their stages' own.  EVERY thread reaches every barrier in every form.

// LDS of k_group_mapped = the value stages (kCmpLdsChunks chunks: 9 344 bytes) + the slice (kMappedSlice bytes + one word
// for the phase of lo) + kMappedBins bins of 12 bytes.  2 048 is the largest power of two that keeps the sum within the
// 18 KiB of the sibling kernels (eight workgroups per CU): 9 344 + 2 056 + 6 144 = 17 544; 4 096 would make 19 592.
constexpr uint32_t kMappedSlice = 2048;
constexpr uint32_t kMappedSliceWords = kMappedSlice / 8 + 1; // 64-bit words: [s0, hi) from any byte phase of lo
constexpr uint32_t kMappedBins = 512;                        // ngroups x copies
constexpr uint32_t kMappedMaxCopies = 64;                    // a lane of its own per copy: more would not spread further
static_assert((kMappedSlice & (kMappedSlice - 1u)) == 0u, "a power of two");
static_assert(kCmpLdsChunks * 16u + kMappedSliceWords * 8u + kMappedBins * 12u <= 18u * 1024u,
              "stage + slice + bins: eight workgroups per CU");
static_assert(kCmpLdsChunks * 16u + (2u * kMappedSlice / 8u + 1u) * 8u + kMappedBins * 12u > 18u * 1024u,
              "... and the largest such power of two");
static_assert(kMappedBins >= 2u * 256u, "two copies of the most groups");

// the copies of `ngroups` bins the budget allows: a power of two (host; the knob group_mapped_copies caps it)
inline uint32_t mapped_copies(uint32_t ngroups, int knob) {
	uint32_t c = 1;
	while (c * 2u * ngroups <= kMappedBins && c * 2u <= kMappedMaxCopies) c *= 2u;
	if (knob > 0) {
		uint32_t k = 1;
		while (k * 2u <= (uint32_t)knob) k *= 2u;
		c = c < k ? c : k;
	}
	return c;
}

struct MappedPlan {
	DensePlan p;  // reader, delta, vframe
	bool slice;
	uint64_t s0;  // slice: the index of byte 0 of the window, a multiple of 8
	uint32_t nw;  // slice: 64-bit words of the window, 1 ... kMappedSliceWords
};

// Uniform; dense_plan's reader, and the indices [lo, hi) the key segment can reach measured against kMappedSlice.
template <bool VAL>
__device__ __forceinline__ MappedPlan mapped_plan(const adac_segment_desc &kd, const MemberDomain &dom,
                                                  const adac_segment_desc &vd, uint64_t v_tmask, uint64_t v_sbit) {
	MappedPlan m {dense_plan<VAL>(kd, dom, vd, v_tmask, v_sbit), false, 0ull, 0u};
	uint64_t add = 0;
	if (m.p.reader == kMemHeader || !product_frame(kd, dom.tmask, dom.sbit, add)) return m;
	const uint64_t bmin = add + dom.sbit, btop = bmin + mask64(kd.width);
	const uint64_t dlo = dom.bbase, dhi = dom.bbase + (dom.set_bits - 1ull);
	const uint64_t lo = bmin > dlo ? bmin - dlo : 0ull;
	const uint64_t hi = (btop < dhi ? btop : dhi) - dlo + 1ull; // <= key_span
	m.slice = hi - lo <= (uint64_t)kMappedSlice;
	m.s0 = lo & ~7ull;
	m.nw = m.slice ? (uint32_t)((hi - m.s0 + 7ull) >> 3) : 0u;
	return m;
}

// d_map -> the window.  The whole workgroup; the caller's barrier follows.  Word index clamped into the allocation of
// ceil(key_span / 8) words; the bytes at indices >= key_span that come along are never looked up.
__device__ __forceinline__ void mapped_slice_fill(const MappedPlan &plan, const uint8_t *__restrict__ map,
                                                  uint64_t key_span, unsigned long long *slice) {
	const unsigned long long *map64 = reinterpret_cast<const unsigned long long *>(map);
	const uint64_t n64 = (key_span + 7ull) >> 3;
	for (uint32_t i = threadIdx.x; i < plan.nw; i += (uint32_t)kWorkgroup) {
		const uint64_t gw = (plan.s0 >> 3) + i;
		slice[i] = map64[gw < n64 ? gw : n64 - 1ull];
	}
}

// The probe's sink.  slice form: every row of the group whose t is in the domain has s0 <= t < s0 + 8 * nw.
template <bool SUM>
struct MappedBins {
	const uint8_t *map;         // d_map
	const uint8_t *slice;       // the LDS window
	unsigned long long *bsum;   // the lane's copy of the LDS bins: sums (SUM) ...
	uint32_t *bcnt;             // ... and counts (when they are wanted)
	uint64_t s0;
	uint32_t ngroups;
	bool in_slice, cnt;         // uniform
	uint64_t osum = 0;          // the overflow entry, in registers
	uint32_t ocnt = 0;
	// a wanted row of index t < key_span and value v
	__device__ __forceinline__ void row(uint64_t t, uint64_t v) {
		const uint32_t g = in_slice ? slice[(uint32_t)(t - s0)] : map[t];
		if (g < ngroups) {
			if (SUM) atomicAdd(&bsum[g], (unsigned long long)v);
			if (cnt) atomicAdd(&bcnt[g], 1u);
		} else {
			if (SUM) osum += v;
			ocnt++;
		}
	}
};

// The build's sink: v is the code widened by the codes column's signedness; as an unsigned number of its own width a
// negative one is above 255.
struct MappedStore {
	uint8_t *map;
	uint64_t c_tmask;
	__device__ __forceinline__ void row(uint64_t t, uint64_t v) {
		const uint64_t c = v & c_tmask;
		map[t] = (uint8_t)(c < 255ull ? c : 255ull);
	}
};

// Reader "walk": dense_walk over a sink.  Rows [r0, r1) of the segment pair, walked by ONE wave: the key column on the
// register walk, the value column's chunks of the same rows staged per wave (VAL only).  `rows` gains the lane's wanted
// rows inside the domain.
template <int W, bool V, bool VAL, class Sink>
__device__ __forceinline__ void mapped_walk(uint32_t r0, uint32_t r1, const adac_segment_desc &kd,
                                            const adac_segment_desc &vd, const uint4 *__restrict__ kseg16,
                                            const uint4 *__restrict__ vseg16, const uint64_t *__restrict__ validity,
                                            uint4 *vstage, const DensePlan &plan, uint64_t key_span, Sink &sink,
                                            uint32_t &rows) {
	constexpr int MAXV = ChunkWindow<W>::MAXV;
	const uint32_t wv = VAL ? vd.width : 1u, vmask32 = mask32(wv);
	// as many lanes as keep the round's rows of the value column inside the buffer (product_walk's bound)
	uint32_t lanes = 64u;
	if (VAL) {
		lanes = ((kProdWaveData - 2u) * 128u) / ((uint32_t)MAXV * wv);
		lanes = lanes < 64u ? lanes : 64u;
	}
	const ChunkRange<W> run(r0, r1, kd.count);
	const uint32_t c0 = run.c0, c1 = run.c1;
	const uint32_t vclast = VAL ? (uint32_t)(((uint64_t)vd.count * wv + 127) >> 7) - 1 : 0u; // last chunk with data bits
	const uint32_t lane = threadIdx.x & 63u;
	const bool walker = lane < lanes;
	uint32_t L = c0 + lane;
	uint4 q;
	uint32_t e;
	run.load(kseg16, L, q, e);
	const ChunkMask<W, V> vmask(validity, kd.val_off, r1); // the keys' element space
	uint64_t vm0 = 0, vm1 = 0;
	if (V) vmask.words(run.clamp(L), vm0, vm1);
	auto round_v = [&](uint32_t rc, uint32_t &vc0, uint32_t &nv) {
		const uint32_t lo = chunk_first_row<W>(rc);
		uint32_t hi = chunk_first_row<W>(rc + lanes);
		hi = hi < r1 ? hi : r1;
		vc0 = (lo * wv) >> 7;
		nv = hi > lo ? ((hi * wv + 127u) >> 7) - vc0 : 0u;
	};
	// (two named chunks, not an array of two: dense_walk records that as an array they went to scratch)
	auto load_v = [&](uint32_t vc0, uint4 &v0, uint4 &v1) { // unconditional, index clamped into the segment
		const uint32_t c = vc0 + lane;
		v0 = vseg16[c < vclast ? c : vclast];
		v1 = vseg16[c + 64u < vclast ? c + 64u : vclast];
	};
	auto store_v = [&](const uint4 &v0, const uint4 &v1, uint32_t nv) {
		if (lane < nv) vstage[lane] = v0;
		if (lane + 64u < nv) vstage[lane + 64u] = v1;
	};
	const uint32_t *v32 = reinterpret_cast<const uint32_t *>(vstage);
	uint32_t vc0 = 0, nv = 0;
	uint4 vq0 = make_uint4(0u, 0u, 0u, 0u), vq1 = vq0;
	if (VAL) {
		round_v(c0, vc0, nv);
		load_v(vc0, vq0, vq1);
		store_v(vq0, vq1, nv);
	}
	for (uint32_t round0 = c0; round0 < c1; round0 += lanes, L += lanes) { // uniform trip count
		uint4 qn;
		uint32_t en;
		run.load(kseg16, L + lanes, qn, en);
		uint64_t vn0 = 0, vn1 = 0;
		if (V) vmask.words(run.clamp(L + lanes), vn0, vn1);
		uint32_t vc0n = 0, nvn = 0;
		if (VAL) {
			round_v(round0 + lanes, vc0n, nvn);
			load_v(vc0n, vq0, vq1);
		}
		if (walker && L < c1) {
			const ChunkWindow<W> cw(q, e, L, r1);
			const uint32_t have = cw.have();
			// rows that exist AND are wanted, as one mask
			uint32_t vb = have >= 32u ? 0xffffffffu : ((1u << have) - 1u);
			if (V) vb &= (uint32_t)vmask.window(vm0, vm1, cw.i0 < r1 ? cw.i0 : r1);
			const uint32_t vbit = VAL ? cw.i0 * wv - 128u * vc0 : 0u; // row i0 of the values inside the staged chunks
#pragma unroll
			for (int j = 0; j < MAXV; j++) {
				const uint64_t t = (uint64_t)field_of<W>(cw.nrm, j) + plan.delta;
				if (((vb >> j) & 1u) != 0u && t < key_span) {
					uint64_t v = 0ull;
					if (VAL) v = (uint64_t)staged_field32(v32, vbit + (uint32_t)j * wv, vmask32) + plan.vframe;
					sink.row(t, v);
					rows++;
				}
			}
		}
		q = qn;
		e = en;
		vm0 = vn0;
		vm1 = vn1;
		if (VAL) {
			store_v(vq0, vq1, nvn); // after this round's reads of the buffer
			vc0 = vc0n;
		}
	}
}

// Reader "staged" with a value column: dense_staged_pair over a sink.  Every thread runs every barrier.
template <bool V, class Sink>
__device__ __forceinline__ uint32_t mapped_staged_pair(const ScanGroup &g, const adac_segment_desc &vd,
                                                       const uint64_t *__restrict__ kwords,
                                                       const uint64_t *__restrict__ vwords, const MemberDomain &dom,
                                                       uint64_t v_tmask, uint64_t v_sbit,
                                                       const uint64_t *__restrict__ validity, uint4 *lds, Sink &sink) {
	uint4 *kstage[2] = {lds, lds + kCmpStageChunks};
	uint4 *vstage[2] = {lds + 2 * kCmpStageChunks, lds + 3 * kCmpStageChunks};
	const adac_segment_desc &kd = g.d;
	const uint32_t tid = threadIdx.x;
	const uint32_t wk = kd.width, wv = vd.width;
	const uint32_t wmax = wk > wv ? wk : wv;
	uint32_t per_stage = ((kCmpStageBytes * 8u - 256u) / (wmax ? wmax : 1u)) & ~(uint32_t)(kWorkgroup - 1);
	per_stage = per_stage < (uint32_t)kWorkgroup ? (uint32_t)kWorkgroup : per_stage;
	const uint4 *k16 = reinterpret_cast<const uint4 *>(kwords + kd.word_off);
	const uint4 *v16 = reinterpret_cast<const uint4 *>(vwords + vd.word_off);
	const uint64_t kadd = effective_add(kd), vadd = effective_add(vd);
	auto make_stage = [&](uint32_t done, CompareStage &st) -> bool {
		if (done >= g.n) return false;
		st.row0 = g.first + done;
		st.m = g.n - done < per_stage ? g.n - done : per_stage;
		const uint64_t apos = (uint64_t)st.row0 * wk, bpos = (uint64_t)st.row0 * wv;
		st.asrc = k16 + (apos >> 7);
		st.bsrc = v16 + (bpos >> 7);
		st.abit0 = (uint32_t)(apos & 127);
		st.bbit0 = (uint32_t)(bpos & 127);
		st.achunks = (st.abit0 + st.m * wk + 127u) >> 7; // <= kCmpStageBytes / 16 + 1: one per thread
		st.bchunks = (st.bbit0 + st.m * wv + 127u) >> 7;
		return true;
	};
	CompareStage cur, nxt;
	uint32_t done = 0;
	bool have = make_stage(done, cur); // uniform
	uint4 kq, vq;
	if (have) {
		if (tid < cur.achunks) kstage[0][tid] = cur.asrc[tid];
		if (tid < cur.bchunks) vstage[0][tid] = cur.bsrc[tid];
	}
	__syncthreads();
	const uint32_t kmlo = wk >= 32u ? 0xffffffffu : mask32(wk), kmhi = wk > 32u ? mask32(wk - 32u) : 0u;
	const uint32_t vmlo = wv >= 32u ? 0xffffffffu : mask32(wv), vmhi = wv > 32u ? mask32(wv - 32u) : 0u;
	uint32_t rows = 0;
	uint32_t buf = 0;
	while (have) { // uniform
		done += cur.m;
		const bool more = make_stage(done, nxt);
		if (more) { // in flight while this stage is consumed: unconditional loads, index clamped into the stage
			kq = nxt.asrc[tid < nxt.achunks ? tid : (nxt.achunks ? nxt.achunks - 1u : 0u)];
			vq = nxt.bsrc[tid < nxt.bchunks ? tid : (nxt.bchunks ? nxt.bchunks - 1u : 0u)];
		}
		const uint32_t *k32 = reinterpret_cast<const uint32_t *>(kstage[buf]);
		const uint32_t *v32 = reinterpret_cast<const uint32_t *>(vstage[buf]);
		const uint64_t elem0 = kd.val_off + cur.row0; // the keys' element space
		for (uint32_t base = 0; base < cur.m; base += (uint32_t)kWorkgroup) { // uniform trip count
			const uint32_t row = base + tid;
			const uint32_t rr = row < cur.m ? row : cur.m - 1u; // clamped: the reads stay inside the stage and the mask
			const uint64_t fk = staged_field(k32, cur.abit0 + rr * wk, kmlo, kmhi);
			const uint64_t fv = staged_field(v32, cur.bbit0 + rr * wv, vmlo, vmhi);
			const uint32_t keep = V ? (validity_window_pair(validity, elem0 + rr, 1u) & 1u) : 1u;
			const uint64_t t = ((((fk + kadd) & dom.tmask) ^ dom.sbit) - dom.bbase);
			uint64_t y = (fv + vadd) & v_tmask;
			y = (y ^ v_sbit) - v_sbit; // widened by the value column's signedness
			if (row < cur.m && keep != 0u && t < dom.set_bits) {
				sink.row(t, y);
				rows++;
			}
		}
		if (more) {
			if (tid < nxt.achunks) kstage[buf ^ 1u][tid] = kq;
			if (tid < nxt.bchunks) vstage[buf ^ 1u][tid] = vq;
		}
		__syncthreads();
		cur = nxt;
		have = more;
		buf ^= 1u;
	}
	return rows;
}

// Reader "staged" without a value column: dense_staged_keys over a sink.  Every thread runs every barrier.
template <bool V, class Sink>
__device__ __forceinline__ uint32_t mapped_staged_keys(const ScanGroup &g, const uint64_t *__restrict__ words,
                                                       const MemberDomain &dom, const uint64_t *__restrict__ validity,
                                                       uint4 *stage, Sink &sink) {
	const adac_segment_desc &d = g.d;
	const uint32_t tid = threadIdx.x;
	const uint32_t w = d.width;
	const uint32_t per_stage = (kMemberStageBits / (w ? w : 1u)) & ~63u; // >= 64 rows
	const uint4 *s16 = reinterpret_cast<const uint4 *>(words + d.word_off);
	const uint64_t add = effective_add(d);
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
		st.chunks = (st.bit0 + st.m * w + 127u) >> 7; // <= kMemberStageChunks - 3
		return true;
	};
	Stage cur, nxt;
	uint32_t done = 0;
	bool have = make_stage(done, cur); // uniform
	uint4 q = make_uint4(0u, 0u, 0u, 0u);
	if (have) q = cur.src[tid < cur.chunks ? tid : (cur.chunks ? cur.chunks - 1u : 0u)];
	uint32_t rows = 0;
	while (have) { // uniform
		if (tid < cur.chunks) stage[tid] = q;
		__syncthreads();
		done += cur.m;
		const bool more = make_stage(done, nxt);
		// in flight while this stage is consumed: an unconditional load, index clamped into the stage
		if (more) q = nxt.src[tid < nxt.chunks ? tid : (nxt.chunks ? nxt.chunks - 1u : 0u)];
		const uint64_t elem0 = d.val_off + cur.row0;
		for (uint32_t base = 0; base < cur.m; base += (uint32_t)kWorkgroup) {
			const uint32_t row = base + tid;
			const uint32_t rr = row < cur.m ? row : cur.m - 1u; // clamped: the reads stay inside the stage and the mask
			const uint64_t f = staged_field(s32, cur.bit0 + rr * w, mlo, mhi);
			const uint32_t keep = V ? (validity_window_pair(validity, elem0 + rr, 1u) & 1u) : 1u;
			const uint64_t t = ((((f + add) & dom.tmask) ^ dom.sbit) - dom.bbase);
			if (row < cur.m && keep != 0u && t < dom.set_bits) {
				sink.row(t, 0ull);
				rows++;
			}
		}
		__syncthreads(); // every thread has read the stage
		cur = nxt;
		have = more;
	}
	return rows;
}

// One scan group through the reader its plan names, into `sink`; returns the thread's wanted rows inside the domain.
// Every thread reaches the staged readers' barriers; a wave whose quarter is empty, and the header form, skip the walk.
template <bool V, bool VAL, class Sink>
__device__ __forceinline__ uint32_t mapped_read(const ScanGroup &g, const adac_segment_desc &vd, const DensePlan &plan,
                                                const uint64_t *__restrict__ kwords,
                                                const uint64_t *__restrict__ vwords, const MemberDomain &dom,
                                                uint64_t v_tmask, uint64_t v_sbit,
                                                const uint64_t *__restrict__ validity, uint4 *lds, Sink &sink) {
	uint32_t rows = 0;
	if (plan.reader == kMemWalk) {
		const uint32_t wave = threadIdx.x >> 6;
		const RwQuarter qr(g, wave);
		if (!qr.empty()) { // uniform per wave; the walk has no barrier
			dispatch_width_4_32(g.d.width, [&](auto wc) __attribute__((always_inline)) {
				mapped_walk<decltype(wc)::value, V, VAL>(qr.r0, qr.r1, g.d, vd,
				                                         reinterpret_cast<const uint4 *>(kwords + g.d.word_off),
				                                         reinterpret_cast<const uint4 *>(vwords + vd.word_off), validity,
				                                         lds + wave * kProdWaveChunks, plan, dom.set_bits, sink, rows);
			});
		}
	} else if (plan.reader == kMemStaged) {
		if constexpr (VAL) {
			rows = mapped_staged_pair<V>(g, vd, kwords, vwords, dom, v_tmask, v_sbit, validity, lds, sink);
		} else {
			rows = mapped_staged_keys<V>(g, kwords, dom, validity, lds, sink);
		}
	}
	return rows;
}

// the rows per segment: one atomicAdd per wave
__device__ __forceinline__ void mapped_seg_rows(unsigned long long *__restrict__ seg_rows, uint32_t seg, uint32_t rows) {
	if (seg_rows) { // uniform
		const uint64_t tot = wave_sum((uint64_t)rows);
		if ((threadIdx.x & 63u) == 0u && tot != 0ull) atomicAdd(seg_rows + seg, (unsigned long long)tot);
	}
}

// Probe.  V: a mask is given; SUM: a value column is read and sums are kept (without: the counts alone).  copies: a
// power of two with copies * ngroups <= kMappedBins (mapped_copies).
template <bool V, bool SUM>
__global__ __launch_bounds__(kWorkgroup) void k_group_mapped(const ScanGroup *__restrict__ kgroups,
                                                             const uint64_t *__restrict__ kwords,
                                                             const adac_segment_desc *__restrict__ vdescs,
                                                             const uint64_t *__restrict__ vwords, MemberDomain dom,
                                                             uint64_t v_tmask, uint64_t v_sbit,
                                                             const uint64_t *__restrict__ validity,
                                                             const uint8_t *__restrict__ map, uint32_t ngroups,
                                                             uint32_t copies, unsigned long long *sums,
                                                             unsigned long long *counts,
                                                             unsigned long long *__restrict__ seg_rows) {
	__shared__ uint4 lds[SUM ? kCmpLdsChunks : kMemberStageChunks];
	__shared__ unsigned long long slice[kMappedSliceWords];
	__shared__ unsigned long long bsum[SUM ? kMappedBins : 1];
	__shared__ uint32_t bcnt[kMappedBins];
	const ScanGroup g = load_scan_group(kgroups, blockIdx.x);
	adac_segment_desc vd = g.d;
	if (SUM) vd = load_desc_scalar(vdescs, g.seg);
	const MappedPlan plan = mapped_plan<SUM>(g.d, dom, vd, v_tmask, v_sbit);
	const bool live = plan.p.reader != kMemHeader; // uniform
	const bool cnt = !SUM || counts != nullptr;    // uniform
	const uint32_t nbins = ngroups * copies;       // <= kMappedBins
	if (live) {
		for (uint32_t i = threadIdx.x; i < nbins; i += (uint32_t)kWorkgroup) {
			if (SUM) bsum[i] = 0ull;
			bcnt[i] = 0u;
		}
		if (plan.slice) mapped_slice_fill(plan, map, dom.set_bits, slice);
	}
	__syncthreads();
	const uint32_t mine = (threadIdx.x & (copies - 1u)) * ngroups; // the lane's copy
	MappedBins<SUM> sink {map, reinterpret_cast<const uint8_t *>(slice), bsum + (SUM ? mine : 0u), bcnt + mine, plan.s0,
	                      ngroups, plan.slice, cnt};
	const uint32_t rows = mapped_read<V, SUM>(g, vd, plan.p, kwords, vwords, dom, v_tmask, v_sbit, validity, lds, sink);
	mapped_seg_rows(seg_rows, g.seg, rows);
	// the overflow entry: one reduction per wave
	const uint64_t osum = SUM ? wave_sum(sink.osum) : 0ull;
	const uint64_t ocnt = wave_sum((uint64_t)sink.ocnt);
	if ((threadIdx.x & 63u) == 0u && ocnt != 0ull) {
		if (SUM && osum != 0ull) atomicAdd(sums + ngroups, (unsigned long long)osum);
		if (cnt) atomicAdd(counts + ngroups, (unsigned long long)ocnt);
	}
	__syncthreads(); // every wave's rows are in the bins
	if (live) {
		for (uint32_t b = threadIdx.x; b < ngroups; b += (uint32_t)kWorkgroup) {
			unsigned long long s = 0ull;
			uint32_t c = 0u;
			for (uint32_t k = 0; k < copies; k++) {
				if (SUM) s += bsum[k * ngroups + b];
				c += bcnt[k * ngroups + b];
			}
			if (SUM && s) atomicAdd(sums + b, s);
			if (cnt && c) atomicAdd(counts + b, (unsigned long long)c);
		}
	}
}

// Build.  V: a mask is given.  The dense pair scan with the accumulator replaced by a byte store; no LDS window.
template <bool V>
__global__ __launch_bounds__(kWorkgroup) void k_build_map(const ScanGroup *__restrict__ kgroups,
                                                          const uint64_t *__restrict__ kwords,
                                                          const adac_segment_desc *__restrict__ cdescs,
                                                          const uint64_t *__restrict__ cwords, MemberDomain dom,
                                                          uint64_t c_tmask, uint64_t c_sbit,
                                                          const uint64_t *__restrict__ validity, uint8_t *map,
                                                          unsigned long long *__restrict__ seg_rows) {
	__shared__ uint4 lds[kCmpLdsChunks];
	const ScanGroup g = load_scan_group(kgroups, blockIdx.x);
	const adac_segment_desc cd = load_desc_scalar(cdescs, g.seg);
	const DensePlan plan = dense_plan<true>(g.d, dom, cd, c_tmask, c_sbit);
	MappedStore sink {map, c_tmask};
	const uint32_t rows = mapped_read<V, true>(g, cd, plan, kwords, cwords, dom, c_tmask, c_sbit, validity, lds, sink);
	mapped_seg_rows(seg_rows, g.seg, rows);
}
