// adac_sum_product.inl — Q6's aggregate: SUM(a * b) over TWO packed columns of the same table under a selection bitmap.
// Included into adac_kernels.hip inside namespace adac::{anonymous}, after adac_group_sum.inl (staged_field,
// load_desc_scalar and the stage geometry are shared with the grouped scan).
//
// One workgroup per ScanGroup of `a`; the rows [g.first, g.first + g.n) are the same rows of `b` (equal counts, segment
// by segment).  Nothing is materialised: each value is widened to 64 bits by its own column's signedness, the product
// and the sum are taken mod 2^64, rows whose bit is clear in the mask (indexed in a's element space) take no part.
// Two forms, chosen per group from the two descriptors and the types alone (product_fast_eligible):
//   fast     both segments linear (or raw and unsigned), 4 <= wa <= 32, wb <= 32: a wave walks a quarter of the group
//            (RwQuarter, adac_group_rw_walk.inl) on its own.  `a` on the fused scans' width-templated register walk (a
//            lane owns whole 16-byte chunks, the
//            next chunk and its mask words requested a round ahead, every field at a compile-time position); the
//            16-byte chunks of `b` that hold the same contiguous row run are staged in a wave-private LDS buffer (the
//            next round's chunks are loaded before this round is walked and stored after it: LDS operations of one
//            wave execute in order, so the loop has no barrier).  The loop works on FIELDS: with frames ma, mb
//              sum (fa + ma)(fb + mb) = sum fa fb + mb sum fa + ma sum fb + n ma mb   (mod 2^64),
//            so a row costs one 32 x 32 -> 64 multiply-add and two masked adds; the frames are applied once per wave.
//   generic  everything else (widths 1..64, all eight types on either side, raw signed, wrapping and unpacked
//            segments, ADAC_NO_MIN, the all-ones stored min): the packed bits of the same rows of both columns staged
//            in LDS with k_group_sum's stage structure, value = (((field + effective_add) & tmask) ^ sbit) - sbit per
//            column, one 64-bit multiply per row, the mask bit looked up per row.
// Result: the caller clears d_sums; every wave adds its total with ONE 64-bit atomicAdd per group (wrapping sums
// commute) — the fused scans' form without arrival cells.  No other global atomics, not persistent.

constexpr uint32_t kProdStageChunks = kGroupStageBytes / 16 + 2; // one stage buffer of one column (generic form)
constexpr uint32_t kProdWaveData = 128;                          // fast form: chunks of b a wave stages per round ...
constexpr uint32_t kProdWaveChunks = kProdWaveData + 18;         // ... + over-read slack (32 rows x 32 bits + a dword)
static_assert(4 * kProdStageChunks >= (kWorkgroup / 64) * kProdWaveChunks, "the two forms share one LDS block");

struct ProductTypes {
	uint64_t a_tmask, a_sbit; // all-ones mask of the type's width, its sign bit (0 for unsigned types)
	uint64_t b_tmask, b_sbit;
};

struct ProductPlan {
	bool ok;
	uint64_t ma, mb; // value64 = field + frame on either side (0 for raw segments)
};

// value64 = field + add for EVERY w-bit field without leaving T's range (frame_fits_type), or the field itself (raw
// slots / no frame of reference, unsigned T)
__device__ __forceinline__ bool product_frame(const adac_segment_desc &d, uint64_t tmask, uint64_t sbit, uint64_t &add) {
	if ((d.flags & ADAC_SEG_PACKED) && d.min != ADAC_NO_MIN) return frame_fits_type(d, tmask, sbit, add);
	add = 0ull;
	return sbit == 0ull;
}

// Uniform; depends on the two descriptors and the types only.
__device__ __forceinline__ ProductPlan product_fast_eligible(const adac_segment_desc &ad, const adac_segment_desc &bd,
                                                             const ProductTypes &ty) {
	ProductPlan p {false, 0ull, 0ull};
	const uint32_t wa = ad.width, wb = bd.width;
	if (wa < 4u || wa > 32u || wb < 1u || wb > 32u) return p;
	if ((uint64_t)ad.count * wa >= (1ull << 31) || (uint64_t)bd.count * wb >= (1ull << 31)) return p;
	if (!product_frame(ad, ty.a_tmask, ty.a_sbit, p.ma) || !product_frame(bd, ty.b_tmask, ty.b_sbit, p.mb)) return p;
	p.ok = true;
	return p;
}

// what a wave keeps of its rows: sums of FIELDS (mod 2^64) and the rows kept
struct ProductAcc {
	uint64_t pp = 0, pa = 0, pb = 0;
	uint32_t rows = 0;
};

// Fast form: rows [r0, r1) of the segment pair, walked by ONE wave (r0 a multiple of 128 rows: its bits start a chunk
// of `a`).  `bstage`: the wave's kProdWaveChunks chunks of LDS.
template <int W, bool V>
__device__ __forceinline__ void product_walk(uint32_t r0, uint32_t r1, const adac_segment_desc &ad,
                                             const adac_segment_desc &bd, const uint4 *__restrict__ aseg16,
                                             const uint4 *__restrict__ bseg16, const uint64_t *__restrict__ validity,
                                             uint4 *bstage, ProductAcc &acc) {
	constexpr int MAXV = ChunkWindow<W>::MAXV;
	const uint32_t wb = bd.width, bmask = mask32(wb);
	// as many lanes as keep the round's rows of b inside the buffer: rows <= lanes * MAXV, so bits <= 126 chunks, which
	// from any bit offset of the first chunk lie in 128 chunks at most (64 lanes unless b is much wider than a)
	uint32_t lanes = ((kProdWaveData - 2u) * 128u) / ((uint32_t)MAXV * wb);
	lanes = lanes < 64u ? lanes : 64u;
	const ChunkRange<W> run(r0, r1, ad.count);
	const uint32_t c0 = run.c0, c1 = run.c1;
	const uint32_t bclast = (uint32_t)(((uint64_t)bd.count * wb + 127) >> 7) - 1; // last chunk holding data bits of b
	const uint32_t lane = threadIdx.x & 63u;
	const bool walker = lane < lanes;
	uint32_t L = c0 + lane;
	uint4 q;
	uint32_t e;
	run.load(aseg16, L, q, e);
	const ChunkMask<W, V> vmask(validity, ad.val_off, r1); // a's element space
	uint64_t vm0 = 0, vm1 = 0;
	if (V) vmask.words(run.clamp(L), vm0, vm1);
	// b: the round that starts at chunk rc of a covers the rows [first row starting in chunk rc, first row starting in
	// chunk rc + lanes) below r1; bc0 = the chunk of b holding the first bit of the first of them, nb chunks in all
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
		// requested before this round is walked: the next chunk of a, its mask words and the next round's chunks of b
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
			// rows that exist AND are kept, as one mask
			uint32_t vb = have >= 32u ? 0xffffffffu : ((1u << have) - 1u);
			if (V) vb &= (uint32_t)vmask.window(vm0, vm1, cw.i0 < r1 ? cw.i0 : r1);
			const uint32_t bbit = cw.i0 * wb - 128u * bc0; // row i0 of b inside the staged chunks
			ChunkSum<W> sa;
			uint64_t pp = 0, sb = 0;
			// eight rows at a time: their fields of b are read together (eight LDS round trips in flight), then consumed
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
						const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)vb, j0 + u, 1); // 0 / -1
						const uint32_t fa = field_of<W>(cw.nrm, j0 + u) & m;
						sa.add(fa);
						sb += fb[u] & m;
						pp += (uint64_t)fa * fb[u]; // v_mad_u64_u32
					}
				}
			}
			acc.pp += pp;
			acc.pa += (uint64_t)sa.p32 + sa.p64;
			acc.pb += sb;
			acc.rows += (uint32_t)__popc(vb);
		}
		q = qn;
		e = en;
		vm0 = vn0;
		vm1 = vn1;
		store_b(bq, nbn); // after this round's reads of the buffer
		bc0 = bc0n;
	}
}

template <bool V>
__device__ __forceinline__ void product_walk_dispatch(uint32_t r0, uint32_t r1, const adac_segment_desc &ad,
                                                      const adac_segment_desc &bd, const uint4 *__restrict__ aseg16,
                                                      const uint4 *__restrict__ bseg16,
                                                      const uint64_t *__restrict__ validity, uint4 *bstage,
                                                      ProductAcc &acc) {
	dispatch_width_4_32(ad.width, [&](auto wc) __attribute__((always_inline)) {
		product_walk<decltype(wc)::value, V>(r0, r1, ad, bd, aseg16, bseg16, validity, bstage, acc);
	});
}

// one stage of the generic form: rows [row0, row0 + m) of the segment pair (all uniform)
struct ProductStage {
	const uint4 *asrc, *bsrc; // the 16-byte chunks holding the first bit of the rows
	uint32_t abit0, bbit0, achunks, bchunks, row0, m;
};

// Generic form: the whole workgroup, the group in stages.  Returns the thread's part of the group's total.
template <bool V>
__device__ __forceinline__ uint64_t product_generic(const ScanGroup &g, const adac_segment_desc &bd,
                                                    const uint64_t *__restrict__ awords,
                                                    const uint64_t *__restrict__ bwords, const ProductTypes &ty,
                                                    const uint64_t *__restrict__ validity, uint4 *lds) {
	// two stage buffers per column: the next stage's chunks are loaded (into registers) before the current stage is
	// consumed and written to the other buffer after it
	uint4 *astage[2] = {lds, lds + kProdStageChunks};
	uint4 *bstage[2] = {lds + 2 * kProdStageChunks, lds + 3 * kProdStageChunks};
	const adac_segment_desc &ad = g.d;
	const uint32_t tid = threadIdx.x;
	const uint32_t wa = ad.width, wb = bd.width;
	const uint32_t wmax = wa > wb ? wa : wb;
	uint32_t per_stage = ((kGroupStageBytes * 8u - 256u) / wmax) & ~(uint32_t)(kWorkgroup - 1);
	per_stage = per_stage < (uint32_t)kWorkgroup ? (uint32_t)kWorkgroup : per_stage;
	const uint4 *a16 = reinterpret_cast<const uint4 *>(awords + ad.word_off);
	const uint4 *b16 = reinterpret_cast<const uint4 *>(bwords + bd.word_off);
	const uint64_t aadd = effective_add(ad), badd = effective_add(bd);
	auto make_stage = [&](uint32_t done, ProductStage &st) -> bool {
		if (done >= g.n) return false;
		st.row0 = g.first + done;
		st.m = g.n - done < per_stage ? g.n - done : per_stage;
		const uint64_t apos = (uint64_t)st.row0 * wa, bpos = (uint64_t)st.row0 * wb;
		st.asrc = a16 + (apos >> 7);
		st.bsrc = b16 + (bpos >> 7);
		st.abit0 = (uint32_t)(apos & 127);
		st.bbit0 = (uint32_t)(bpos & 127);
		st.achunks = (st.abit0 + st.m * wa + 127u) >> 7; // <= kGroupStageBytes / 16 + 1 <= two per thread, >= 1
		st.bchunks = (st.bbit0 + st.m * wb + 127u) >> 7;
		return true;
	};
	ProductStage cur, nxt;
	uint32_t done = 0;
	bool have = make_stage(done, cur); // uniform
	uint4 aq[kGroupChunksPerThread], bq[kGroupChunksPerThread];
	if (have) {
#pragma unroll
		for (uint32_t h = 0; h < kGroupChunksPerThread; h++) {
			const uint32_t c = tid + h * kWorkgroup;
			if (c < cur.achunks) astage[0][c] = cur.asrc[c];
			if (c < cur.bchunks) bstage[0][c] = cur.bsrc[c];
		}
	}
	__syncthreads();
	const uint32_t amlo = wa >= 32u ? 0xffffffffu : mask32(wa), amhi = wa > 32u ? mask32(wa - 32u) : 0u;
	const uint32_t bmlo = wb >= 32u ? 0xffffffffu : mask32(wb), bmhi = wb > 32u ? mask32(wb - 32u) : 0u;
	uint64_t acc = 0;
	uint32_t buf = 0;
	while (have) {
		done += cur.m;
		const bool more = make_stage(done, nxt);
		if (more) { // in flight while this stage is consumed: unconditional loads, index clamped into the stage
#pragma unroll
			for (uint32_t h = 0; h < kGroupChunksPerThread; h++) {
				const uint32_t c = tid + h * kWorkgroup;
				aq[h] = nxt.asrc[c < nxt.achunks ? c : nxt.achunks - 1u];
				bq[h] = nxt.bsrc[c < nxt.bchunks ? c : nxt.bchunks - 1u];
			}
		}
		const uint32_t *a32 = reinterpret_cast<const uint32_t *>(astage[buf]);
		const uint32_t *b32 = reinterpret_cast<const uint32_t *>(bstage[buf]);
		const uint64_t elem0 = ad.val_off + cur.row0; // a's element space
		for (uint32_t row0 = tid; row0 < cur.m; row0 += 4u * kWorkgroup) {
			uint64_t fa[4], fb[4];
			uint32_t keep[4];
#pragma unroll
			for (int u = 0; u < 4; u++) {
				const uint32_t row = row0 + (uint32_t)u * kWorkgroup;
				const uint32_t rr = row < cur.m ? row : row0; // clamped: the reads stay inside the stage and the mask
				fa[u] = staged_field(a32, cur.abit0 + rr * wa, amlo, amhi);
				fb[u] = staged_field(b32, cur.bbit0 + rr * wb, bmlo, bmhi);
				keep[u] = V ? (validity_window_pair(validity, elem0 + rr, 1u) & 1u) : 1u;
			}
#pragma unroll
			for (int u = 0; u < 4; u++) {
				const uint32_t row = row0 + (uint32_t)u * kWorkgroup;
				uint64_t x = (fa[u] + aadd) & ty.a_tmask;
				x = (x ^ ty.a_sbit) - ty.a_sbit; // widened by a's signedness
				uint64_t y = (fb[u] + badd) & ty.b_tmask;
				y = (y ^ ty.b_sbit) - ty.b_sbit;
				if (row < cur.m && keep[u]) acc += x * y;
			}
		}
		if (more) {
#pragma unroll
			for (uint32_t h = 0; h < kGroupChunksPerThread; h++) {
				const uint32_t c = tid + h * kWorkgroup;
				if (c < nxt.achunks) astage[buf ^ 1u][c] = aq[h];
				if (c < nxt.bchunks) bstage[buf ^ 1u][c] = bq[h];
			}
		}
		__syncthreads();
		cur = nxt;
		have = more;
		buf ^= 1u;
	}
	return acc;
}

template <bool V>
__global__ __launch_bounds__(kWorkgroup) void k_scan_product(const ScanGroup *__restrict__ agroups,
                                                             const uint64_t *__restrict__ awords,
                                                             const adac_segment_desc *__restrict__ bdescs,
                                                             const uint64_t *__restrict__ bwords, ProductTypes ty,
                                                             const uint64_t *__restrict__ validity,
                                                             unsigned long long *__restrict__ sums) {
	__shared__ uint4 lds[4 * kProdStageChunks];
	const ScanGroup g = load_scan_group(agroups, blockIdx.x);
	const adac_segment_desc bd = load_desc_scalar(bdescs, g.seg);
	const ProductPlan plan = product_fast_eligible(g.d, bd, ty);
	uint64_t tot;
	if (plan.ok) { // uniform
		const uint32_t wave = threadIdx.x >> 6;
		const RwQuarter qr(g, wave);
		if (qr.empty()) return; // uniform per wave; no barrier follows
		ProductAcc acc;
		product_walk_dispatch<V>(qr.r0, qr.r1, g.d, bd, reinterpret_cast<const uint4 *>(awords + g.d.word_off),
		                         reinterpret_cast<const uint4 *>(bwords + bd.word_off), validity,
		                         lds + wave * kProdWaveChunks, acc);
		const uint64_t pp = wave_sum(acc.pp), pa = wave_sum(acc.pa), pb = wave_sum(acc.pb);
		const uint64_t n = wave_sum((uint64_t)acc.rows);
		tot = pp + plan.mb * pa + plan.ma * pb + n * plan.ma * plan.mb; // the frames, once per wave
	} else {
		tot = wave_sum(product_generic<V>(g, bd, awords, bwords, ty, validity, lds));
	}
	if ((threadIdx.x & 63u) == 0u && tot != 0ull) atomicAdd(sums + g.seg, (unsigned long long)tot);
}
