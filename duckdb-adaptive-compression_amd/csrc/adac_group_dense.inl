// adac_group_dense.inl — SUM(value), COUNT(*) GROUP BY a DENSE INTEGER KEY of any cardinality over two packed columns of
// one table (TPC-H Q18's SUM(l_quantity) GROUP BY l_orderkey, Q13's COUNT(*) GROUP BY o_custkey), nothing decoded to
// memory and no hash table: the results are arrays indexed by key - key_base.  Included into adac_kernels.hip inside
// namespace adac::{anonymous}, after adac_scan_member.inl: the kernel has k_scan_member_build's shell (one workgroup
// per ScanGroup of the KEY layout, the host clears the outputs, one atomicAdd per wave for the rows per segment, not
// persistent, no arrival cells), the member scans' domain (MemberDomain: t = (bits(k) ^ sbit) - (bits(key_base) ^ sbit),
// in the domain iff t < key_span) and k_scan_compare's second column (the value column's descriptor through
// load_desc_scalar, its chunks staged per wave or per workgroup).
//
// A scan group is handled by one READER and one ACCUMULATOR, both chosen uniformly from the two descriptors, the two
// types and the domain alone (dense_plan; forms.dense_form_groups is its host mirror):
//   header   the key segment has a frame (product_frame) and [frame, frame + 2^w - 1] does not meet the domain: no row
//            can contribute.  No packed word of either column and no mask word is read, nothing is added.
//   walk     key: frame, 4 <= w <= 32, count * w < 2^31 (member_plan's walk); with SUM the value column also needs a
//            frame, 1 <= w <= 32 and count * w < 2^31.  The KEY column on the width-templated register walk, one wave
//            per RwQuarter; the value column's chunks of the same rows staged per wave exactly as compare_walk stages
//            `b`.  Per row t = field_key + delta, the domain test, v = field_value + frame_value (64-bit two's
//            complement).  Without SUM there is no stage and no value load at all.
//   staged   everything else (key widths 1..3 and 33..64, value widths above 32, raw signed slots, ADAC_NO_MIN,
//            unpacked segments, frames that wrap, the all-ones stored min): the whole workgroup, the group in stages of
//            packed bytes in LDS: compare_generic's two-column stages with SUM, member_staged's one-column stage
//            without; the value widened as in compare_generic, t as in member_staged.
//   window   the key segment has a frame and the indices its interval can reach, [lo, hi), are at most kDenseWindow:
//            the workgroup keeps a zeroed LDS window of 64-bit sums and 32-bit counts, rows add into it with LDS
//            atomics, and after the last barrier its non-zero entries go out with one global atomicAdd each.
//   direct   otherwise: global atomicAdd on d_sums + t (and d_counts + t), only when t < key_span: no out-of-range
//            address is ever formed.
//
// RUN COMBINING (walk reader, either accumulator; tuning knob group_dense_combine): a lane visits its chunk's rows in row
// order and keeps (t_cur, sum, count) in registers.  A wanted in-domain row with t == t_cur adds into the registers,
// any other wanted in-domain row flushes the pair with one atomic per output array and starts a new run, the end of the
// chunk flushes.  Masked-out rows and rows outside the domain neither flush nor join a run.  On sorted keys (l_orderkey:
// about four rows per key) that is one atomic per run and chunk where adac_scan_build_member pays one per row.  Integer
// sums mod 2^64 commute, so the results depend neither on the knob nor on the order the atomics arrive in.
//
// Barriers: one after the window is zeroed, one before it is written out; the staged reader has its stages' own.  EVERY
// thread reaches every barrier in every form: the reader is chosen uniformly per workgroup, a wave whose quarter is
// empty, and the header form, skip only the walk.

// The window's entries.  LDS of the kernel = the value stages (kCmpLdsChunks chunks: 9 344 bytes, the walk's four
// per-wave stages; the staged reader's four buffers fit inside) + 12 bytes per entry.  512 is the largest power of two
// that keeps the sum within the 18 KiB of the sibling kernels (eight workgroups per CU): 9 344 + 6 144 = 15 488;
// 1 024 entries would make 21 632.  Every key segment of w <= 9, and every domain of at most 512 keys, takes the window.
constexpr uint32_t kDenseWindow = 512;
static_assert((kDenseWindow & (kDenseWindow - 1u)) == 0u, "a power of two");
static_assert(kCmpLdsChunks * 16u + kDenseWindow * 12u <= 18u * 1024u, "stage + window: eight workgroups per CU");
static_assert(kCmpLdsChunks * 16u + 2u * kDenseWindow * 12u > 18u * 1024u, "... and the largest such power of two");
static_assert(kMemberStageChunks <= kCmpLdsChunks, "the one-column stage fits the same block");

struct DensePlan {
	uint32_t reader; // kMemHeader / kMemWalk / kMemStaged
	bool window;
	uint64_t delta;  // walk: (key frame ^ sbit) - bbase, so that t = field + delta
	uint64_t lo;     // window: the index of its entry 0
	uint32_t nw;     // window: its entries, 1 ... kDenseWindow
	uint64_t vframe; // walk with SUM: value64 = field + vframe
};

// Uniform; depends on the two descriptors, the two types and the domain only.  member_plan (reader of the key, [lo, hi))
// extended by the value column's eligibility for the walk.
template <bool SUM>
__device__ __forceinline__ DensePlan dense_plan(const adac_segment_desc &kd, const MemberDomain &dom,
                                                const adac_segment_desc &vd, uint64_t v_tmask, uint64_t v_sbit) {
	DensePlan p {kMemStaged, false, 0ull, 0ull, 0u, 0ull};
	uint64_t add = 0;
	if (!product_frame(kd, dom.tmask, dom.sbit, add)) return p;
	// biased by the sign bit every interval is one of unsigned numbers below 2^64; neither end wraps
	const uint64_t bmin = add + dom.sbit, btop = bmin + mask64(kd.width);
	const uint64_t dlo = dom.bbase, dhi = dom.bbase + (dom.set_bits - 1ull);
	if (btop < dlo || dhi < bmin) {
		p.reader = kMemHeader;
		return p;
	}
	const uint64_t lo = bmin > dlo ? bmin - dlo : 0ull;         // indices [lo, hi) are what the segment can reach
	const uint64_t hi = (btop < dhi ? btop : dhi) - dlo + 1ull; // <= key_span
	p.window = hi - lo <= (uint64_t)kDenseWindow;
	p.lo = lo;
	p.nw = p.window ? (uint32_t)(hi - lo) : 0u;
	p.delta = bmin - dlo;
	bool walk = kd.width >= 4u && kd.width <= 32u && (uint64_t)kd.count * kd.width < (1ull << 31);
	if (SUM && walk) {
		walk = vd.width >= 1u && vd.width <= 32u && (uint64_t)vd.count * vd.width < (1ull << 31) &&
		       product_frame(vd, v_tmask, v_sbit, p.vframe);
	}
	if (walk) p.reader = kMemWalk;
	return p;
}

// Where the rows' contributions go, for both readers.  window form: every row of the group whose t is in the domain
// has lo <= t < lo + nw (its field has w bits, whatever the row holds).
template <bool SUM>
struct DenseAcc {
	unsigned long long *wsum;   // the LDS window: sums (SUM) ...
	uint32_t *wcnt;             // ... and counts (when d_counts is given)
	unsigned long long *sums;   // d_sums (SUM)
	unsigned long long *counts; // d_counts, or null
	uint64_t lo;
	bool window;                // uniform
	// n > 0 rows of index t < key_span, their values adding up to s
	__device__ __forceinline__ void add(uint64_t t, uint64_t s, uint32_t n) const {
		if (window) {
			const uint32_t r = (uint32_t)(t - lo);
			if (SUM) atomicAdd(&wsum[r], (unsigned long long)s);
			if (!SUM || counts) atomicAdd(&wcnt[r], n);
		} else {
			if (SUM) atomicAdd(sums + t, (unsigned long long)s);
			if (!SUM || counts) atomicAdd(counts + t, (unsigned long long)n);
		}
	}
};

// after the last barrier: the window's non-zero entries -> d_sums / d_counts
template <bool SUM>
__device__ __forceinline__ void dense_window_flush(const DensePlan &plan, const DenseAcc<SUM> &acc) {
	const bool cnt = !SUM || acc.counts; // uniform
	for (uint32_t i = threadIdx.x; i < plan.nw; i += (uint32_t)kWorkgroup) {
		if (SUM) {
			const unsigned long long s = acc.wsum[i];
			if (s) atomicAdd(acc.sums + plan.lo + i, s);
		}
		if (cnt) {
			const uint32_t c = acc.wcnt[i];
			if (c) atomicAdd(acc.counts + plan.lo + i, (unsigned long long)c);
		}
	}
}

// A lane's run of equal keys (RUN COMBINING above).  row(): a wanted row whose index t is in the domain.
template <bool SUM>
struct DenseRun {
	uint64_t t_cur = 0, sum = 0;
	uint32_t n = 0;
	__device__ __forceinline__ void flush(const DenseAcc<SUM> &acc) {
		if (n) acc.add(t_cur, sum, n);
		sum = 0ull;
		n = 0u;
	}
	__device__ __forceinline__ void row(const DenseAcc<SUM> &acc, uint64_t t, uint64_t v, bool combine) {
		if (n != 0u && (t != t_cur || !combine)) flush(acc);
		t_cur = t;
		if (SUM) sum += v;
		n++;
	}
};

// Reader "walk": rows [r0, r1) of the segment pair, walked by ONE wave: member_walk's key column, compare_walk's stage
// of the second one (SUM only).  `rows` gains the lane's wanted rows inside the domain.
template <int W, bool V, bool SUM>
__device__ __forceinline__ void dense_walk(uint32_t r0, uint32_t r1, const adac_segment_desc &kd,
                                           const adac_segment_desc &vd, const uint4 *__restrict__ kseg16,
                                           const uint4 *__restrict__ vseg16, const uint64_t *__restrict__ validity,
                                           uint4 *vstage, const DensePlan &plan, uint64_t key_span, bool combine,
                                           const DenseAcc<SUM> &acc, uint32_t &rows) {
	constexpr int MAXV = ChunkWindow<W>::MAXV;
	const uint32_t wv = SUM ? vd.width : 1u, vmask32 = mask32(wv);
	// as many lanes as keep the round's rows of the value column inside the buffer (product_walk's bound)
	uint32_t lanes = 64u;
	if (SUM) {
		lanes = ((kProdWaveData - 2u) * 128u) / ((uint32_t)MAXV * wv);
		lanes = lanes < 64u ? lanes : 64u;
	}
	const ChunkRange<W> run(r0, r1, kd.count);
	const uint32_t c0 = run.c0, c1 = run.c1;
	const uint32_t vclast = SUM ? (uint32_t)(((uint64_t)vd.count * wv + 127) >> 7) - 1 : 0u; // last chunk with data bits
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
	// (two named chunks, not compare_walk's array of two: as an array they went to scratch at the widest unrolls)
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
	if (SUM) {
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
		if (SUM) {
			round_v(round0 + lanes, vc0n, nvn);
			load_v(vc0n, vq0, vq1);
		}
		if (walker && L < c1) {
			const ChunkWindow<W> cw(q, e, L, r1);
			const uint32_t have = cw.have();
			// rows that exist AND are wanted, as one mask
			uint32_t vb = have >= 32u ? 0xffffffffu : ((1u << have) - 1u);
			if (V) vb &= (uint32_t)vmask.window(vm0, vm1, cw.i0 < r1 ? cw.i0 : r1);
			const uint32_t vbit = SUM ? cw.i0 * wv - 128u * vc0 : 0u; // row i0 of the values inside the staged chunks
			DenseRun<SUM> dr;
#pragma unroll
			for (int j = 0; j < MAXV; j++) {
				const uint64_t t = (uint64_t)field_of<W>(cw.nrm, j) + plan.delta;
				if (((vb >> j) & 1u) != 0u && t < key_span) {
					uint64_t v = 0ull;
					if (SUM) v = (uint64_t)staged_field32(v32, vbit + (uint32_t)j * wv, vmask32) + plan.vframe;
					dr.row(acc, t, v, combine);
					rows++;
				}
			}
			dr.flush(acc);
		}
		q = qn;
		e = en;
		vm0 = vn0;
		vm1 = vn1;
		if (SUM) {
			store_v(vq0, vq1, nvn); // after this round's reads of the buffer
			vc0 = vc0n;
		}
	}
}

// Reader "staged" with a value column: the whole workgroup, the group in stages (compare_generic's structure: two
// buffers per column, the next stage in flight while this one is consumed).  Every thread runs every barrier.
template <bool V>
__device__ __forceinline__ uint32_t dense_staged_pair(const ScanGroup &g, const adac_segment_desc &vd,
                                                      const uint64_t *__restrict__ kwords,
                                                      const uint64_t *__restrict__ vwords, const MemberDomain &dom,
                                                      uint64_t v_tmask, uint64_t v_sbit,
                                                      const uint64_t *__restrict__ validity, uint4 *lds,
                                                      const DenseAcc<true> &acc) {
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
				acc.add(t, y, 1u);
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

// Reader "staged" without a value column: member_staged's one-column stage (one buffer: the next stage's chunks are
// loaded while this one is consumed and stored between two barriers).  Every thread runs every barrier.
template <bool V>
__device__ __forceinline__ uint32_t dense_staged_keys(const ScanGroup &g, const uint64_t *__restrict__ words,
                                                      const MemberDomain &dom, const uint64_t *__restrict__ validity,
                                                      uint4 *stage, const DenseAcc<false> &acc) {
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
				acc.add(t, 0ull, 1u);
				rows++;
			}
		}
		__syncthreads(); // every thread has read the stage
		cur = nxt;
		have = more;
	}
	return rows;
}

// The body.  V: a mask is given; SUM: a value column is read and sums are kept.  window_ok / combine: the tuning knobs
// group_dense_window and group_dense_combine.
template <bool V, bool SUM>
__device__ __forceinline__ void dense_scan(const ScanGroup *__restrict__ groups, const uint64_t *__restrict__ kwords,
                                           const adac_segment_desc *__restrict__ vdescs,
                                           const uint64_t *__restrict__ vwords, const MemberDomain &dom, uint64_t v_tmask,
                                           uint64_t v_sbit, const uint64_t *__restrict__ validity,
                                           unsigned long long *sums, unsigned long long *counts,
                                           unsigned long long *__restrict__ seg_rows, uint32_t knobs, uint4 *lds,
                                           unsigned long long *wsum, uint32_t *wcnt) {
	const ScanGroup g = load_scan_group(groups, blockIdx.x);
	adac_segment_desc vd = g.d;
	if (SUM) vd = load_desc_scalar(vdescs, g.seg);
	DensePlan plan = dense_plan<SUM>(g.d, dom, vd, v_tmask, v_sbit);
	if (!(knobs & 2u)) plan.window = false; // uniform
	const bool combine = (knobs & 1u) != 0u;
	const DenseAcc<SUM> acc {wsum, wcnt, sums, counts, plan.lo, plan.window};
	const bool live = plan.reader != kMemHeader; // uniform
	if (live && plan.window) {
		for (uint32_t i = threadIdx.x; i < plan.nw; i += (uint32_t)kWorkgroup) {
			if (SUM) wsum[i] = 0ull;
			wcnt[i] = 0u;
		}
	}
	__syncthreads();
	uint32_t rows = 0;
	if (plan.reader == kMemWalk) {
		const uint32_t wave = threadIdx.x >> 6;
		const RwQuarter qr(g, wave);
		if (!qr.empty()) { // uniform per wave; the walk has no barrier, the ones below are reached by every wave
			dispatch_width_4_32(g.d.width, [&](auto wc) __attribute__((always_inline)) {
				dense_walk<decltype(wc)::value, V, SUM>(qr.r0, qr.r1, g.d, vd,
				                                        reinterpret_cast<const uint4 *>(kwords + g.d.word_off),
				                                        reinterpret_cast<const uint4 *>(vwords + vd.word_off), validity,
				                                        lds + wave * kProdWaveChunks, plan, dom.set_bits, combine, acc,
				                                        rows);
			});
		}
	} else if (plan.reader == kMemStaged) {
		if constexpr (SUM) {
			rows = dense_staged_pair<V>(g, vd, kwords, vwords, dom, v_tmask, v_sbit, validity, lds, acc);
		} else {
			rows = dense_staged_keys<V>(g, kwords, dom, validity, lds, acc);
		}
	}
	if (seg_rows) { // uniform
		const uint64_t tot = wave_sum((uint64_t)rows);
		if ((threadIdx.x & 63u) == 0u && tot != 0ull) atomicAdd(seg_rows + g.seg, (unsigned long long)tot);
	}
	__syncthreads(); // every wave's rows are in the window
	if (live && plan.window) dense_window_flush<SUM>(plan, acc);
}

// V: a mask is given; SUM: a value column is read and sums are kept (without: the counts alone).
template <bool V, bool SUM>
__global__ __launch_bounds__(kWorkgroup) void k_group_dense(const ScanGroup *__restrict__ kgroups,
                                                            const uint64_t *__restrict__ kwords,
                                                            const adac_segment_desc *__restrict__ vdescs,
                                                            const uint64_t *__restrict__ vwords, MemberDomain dom,
                                                            uint64_t v_tmask, uint64_t v_sbit,
                                                            const uint64_t *__restrict__ validity,
                                                            unsigned long long *sums, unsigned long long *counts,
                                                            unsigned long long *__restrict__ seg_rows, uint32_t knobs) {
	__shared__ uint4 lds[SUM ? kCmpLdsChunks : kMemberStageChunks];
	__shared__ unsigned long long wsum[SUM ? kDenseWindow : 1];
	__shared__ uint32_t wcnt[kDenseWindow];
	dense_scan<V, SUM>(kgroups, kwords, vdescs, vwords, dom, v_tmask, v_sbit, validity, sums, counts, seg_rows, knobs, lds,
	                   wsum, wcnt);
}
