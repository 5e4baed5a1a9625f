// adac_dense_read.inl — the READERS of the dense-key scans (k_group_dense, k_group_mapped, k_build_map): how the rows of
// one scan group of the KEY layout, and of the value column's segment of the same rows, are visited, stated once.
// Included by adac_group_dense.inl right after DensePlan / dense_plan, which choose the reader; what a row does once it
// is found is the caller's SINK.
//
//   walk     dense_key_walk: the KEY column on the width-templated register walk, one wave per RwQuarter; the value
//            column's chunks of the same rows staged per wave exactly as compare_walk stages `b` (VAL only: without a
//            value column there is no stage and no value load at all).  Per row t = field_key + delta, the domain test,
//            v = field_value + frame_value (64-bit two's complement).  No barrier.
//   staged   the whole workgroup, the group in stages of packed bytes in LDS: dense_key_staged_pair with a value column
//            (compare_generic's two-column stages, the value widened by its column's signedness), dense_key_staged_keys
//            without (member_staged's one-column stage); t as in member_staged.  Every thread runs every barrier.
//   header   no reader: no packed word of either column and no mask word is read.
//
// THE SINK is any object with
//   row(t, v)   a wanted row (it exists, and the mask, if there is one, keeps it) whose index t is in the domain,
//               t < key_span; v is its value as a 64-bit two's-complement number, 0 without a value column.  Nothing
//               else reaches the sink: no out-of-range t is ever handed over.
//   end()       the rows this lane visits consecutively, in row order, stop here: whatever row() kept back to combine
//               with a neighbour has to leave now.  The walk calls it once after a chunk's rows, in the lanes that
//               walked a chunk.  The staged readers call it after EVERY row(): a thread's rows there are 256 apart and
//               never form a run.  A sink that keeps nothing back has an empty end().
// The sink is taken by reference and may keep state in registers (a run, an overflow entry); the readers neither copy
// it nor look into it.  dense_key_read returns the thread's count of row() calls, dense_key_seg_rows sends it out.
//
// The two-value-column walk and the three-column staged reader of adac_group_mapped_product.inl are functions of their
// own (adac_group_rw_walk.inl's rule: never a walk templated over the NUMBER of columns; VAL here is whether there is
// one), and so are the member scans' readers, whose rows leave through ballots and a bitmap image, not through a sink.

// Reader "walk".  Rows [r0, r1) of the segment pair, walked by ONE wave: member_walk's key column, compare_walk's stage
// of the second one (VAL only).  `rows` gains the lane's wanted rows inside the domain.
template <int W, bool V, bool VAL, class Sink>
__device__ __forceinline__ void dense_key_walk(uint32_t r0, uint32_t r1, const adac_segment_desc &kd,
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
			sink.end(); // the lane's next chunk is `lanes` chunks on
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

// Reader "staged" with a value column: the whole workgroup, the group in stages (compare_generic's structure: two
// buffers per column, the next stage in flight while this one is consumed).  Every thread runs every barrier.
template <bool V, class Sink>
__device__ __forceinline__ uint32_t dense_key_staged_pair(const ScanGroup &g, const adac_segment_desc &vd,
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
				sink.end();
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
template <bool V, class Sink>
__device__ __forceinline__ uint32_t dense_key_staged_keys(const ScanGroup &g, const uint64_t *__restrict__ words,
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
				sink.end();
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
__device__ __forceinline__ uint32_t dense_key_read(const ScanGroup &g, const adac_segment_desc &vd, const DensePlan &plan,
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
				dense_key_walk<decltype(wc)::value, V, VAL>(qr.r0, qr.r1, g.d, vd,
				                                            reinterpret_cast<const uint4 *>(kwords + g.d.word_off),
				                                            reinterpret_cast<const uint4 *>(vwords + vd.word_off),
				                                            validity, lds + wave * kProdWaveChunks, plan, dom.set_bits,
				                                            sink, rows);
			});
		}
	} else if (plan.reader == kMemStaged) {
		if constexpr (VAL) {
			rows = dense_key_staged_pair<V>(g, vd, kwords, vwords, dom, v_tmask, v_sbit, validity, lds, sink);
		} else {
			rows = dense_key_staged_keys<V>(g, kwords, dom, validity, lds, sink);
		}
	}
	return rows;
}

// the rows per segment: one atomicAdd per wave
__device__ __forceinline__ void dense_key_seg_rows(unsigned long long *__restrict__ seg_rows, uint32_t seg,
                                                   uint32_t rows) {
	if (seg_rows) { // uniform
		const uint64_t tot = wave_sum((uint64_t)rows);
		if ((threadIdx.x & 63u) == 0u && tot != 0ull) atomicAdd(seg_rows + seg, (unsigned long long)tot);
	}
}
