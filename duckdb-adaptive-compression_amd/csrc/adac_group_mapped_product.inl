// adac_group_mapped_product.inl — SUM(a * b), SUM(a), COUNT(*) GROUP BY A CODE LOOKED UP THROUGH A DENSE KEY over THREE
// packed columns of one table: the two terms of TPC-H's revenue, SUM(l_extendedprice * (1 - l_discount)) per nation of
// the supplier behind l_suppkey (Q5; Q7 - Q10, Q3, Q14, Q19 through their own keys).  With integer decimals
//   revenue[g] = 100 * SUM(price)[g] - SUM(price * disc)[g] = 100 * d_sums_a[g] - d_sums_ab[g]   (mod 2^64),
// both sums from ONE scan.  Nothing is decoded to memory, there is no hash table, no materialised code column and no
// global atomic per row.  Included into adac_kernels.hip inside namespace adac::{anonymous}, after adac_group_mapped.inl,
// whose plan (mapped_plan: header / walk / staged and slice / direct), slice fill and copies rule (mapped_copies against
// kMappedProductBins) are used as they are, as are adac_dense_read.inl's rows per segment (dense_key_seg_rows).  The
// readers are this file's own: that file's walk and staged pair reader have ONE value column, and a walk is never
// templated over the number of columns (adac_group_rw_walk.inl), so the walk with two staged columns and the staged
// reader with three are functions of their own here, and their sink's row() takes both values.
//
// Semantics: k_group_mapped's with the value replaced by a product.  Each factor is widened to 64 bits by its own
// column's signedness, the product and the sums are taken mod 2^64 (adac_scan_sum_product's rule); a wanted row inside
// the domain with g = d_map[t] adds a * b, a and 1 to entry min(g, ngroups) of the three outputs.
//
// Forms, uniform per scan group of the KEY layout (forms.mapped_product_form_groups is the host mirror):
//   header   as k_group_mapped: the key segment's interval misses the domain.  No packed word of any of the three
//            columns, no mask word and no map byte is read.
//   walk     the key as in k_group_mapped (a frame, 4 <= w <= 32, count * w < 2^31) AND both a and b with a frame
//            (product_frame), 1 <= w <= 32 and count * w < 2^31.  The key on the width-templated register walk, one wave
//            per RwQuarter; the chunks of a AND of b that hold the round's rows each staged in a wave-private buffer
//            (requested a round ahead, stored after the round's reads: LDS operations of one wave execute in order, no
//            barrier in the loop), the way k_group_product3_rw holds bstage and cstage.  Lanes per round: as many as
//            keep the round's rows of BOTH staged columns inside their buffers, product_walk's bound at max(w_a, w_b);
//            each column's chunk index is clamped against its own last chunk.  Per row t = field_key + delta, the
//            domain test, va = field_a + frame_a and vb = field_b + frame_b as 64-bit two's-complement numbers, va * vb.
//   staged   everything else: the whole workgroup, the three columns in double-buffered stages of packed bytes
//            (dense_key_staged_pair with a third column), per_stage from the widest of the three.
//   slice / direct for the look-up: unchanged (mapped_plan).
//
// Bins: ngroups x copies entries of {sum_ab, sum_a: 64 bits, count: 32 bits} in LDS, the copy chosen by lane id, so that
// the LDS atomics of lanes that meet in one hot code (a filtered join sends most surviving rows to a few nations) spread
// over `copies` addresses; a row costs two ds_add_u64 and one ds_add_u32 without return, none of which the wave waits
// for.  The overflow entry (osum_ab, osum_a, ocnt), where the filter sends most rows, is kept in registers and leaves
// through one wave reduction.  After the last barrier thread g adds up the copies of bin g and sends a non-zero total
// out with ONE global atomicAdd per output array.  Integer sums mod 2^64 commute: the results depend neither on the
// copies nor on the order of arrival.
//
// LDS: two per-wave walk stages (2 x kCmpLdsChunks chunks = 2 x 9 344 bytes; the staged reader's six buffers of
// kCmpStageChunks chunks fit inside) + the slice (2 056) + kMappedProductBins bins of 20 bytes.  That cannot stay inside
// the siblings' 18 KiB.  512 bins (two copies at 256 groups, 64 at <= 8) make 18 688 + 2 056 + 10 240 = 30 984 bytes:
// FIVE workgroups per CU of the 160 KiB (five waves per SIMD, which the kernel's registers have to allow: at most 96
// VGPRs; the four instantiations take 72 - 80, and __launch_bounds__ holds the compiler to it).  Without d_sums_a the
// second sum array is not declared: 26 896 bytes, six workgroups.  1 024 bins would make 41 224 bytes and three
// workgroups; fewer than 512 would leave 256 groups one copy.  Five waves per SIMD are what hides the latency here: a
// row's map byte (the direct form) is a dependent global load, and its two or three LDS atomics return nothing, so a wave
// waits on memory, not on the bins; ds_add_u64 on one address serialises only among the lanes of one instruction that
// meet there, which is what the copies spread.
//
// Barriers: one after the bins are zeroed and the slice is filled, one before the bins are written out; the staged
// reader has its stages' own.  EVERY thread reaches every barrier in every form.

constexpr uint32_t kMappedProductBins = 512;       // ngroups x copies
constexpr uint32_t kMappedProductResident = 5;     // workgroups per CU = waves per SIMD
constexpr uint32_t kMappedProductLds = 2u * kCmpLdsChunks * 16u + kMappedSliceWords * 8u + kMappedProductBins * 20u;
static_assert(kMappedProductBins >= 2u * 256u, "two copies of the most groups");
static_assert(kMappedProductLds * kMappedProductResident <= 160u * 1024u, "stages + slice + bins: five workgroups per CU");
static_assert(6u * kCmpStageChunks <= 2u * kCmpLdsChunks, "the staged reader's six buffers fit the walk's block");

struct MappedProductPlan {
	MappedPlan m;    // reader (with a as the value column: p.vframe is a's frame), delta, slice
	uint64_t bframe; // walk: value64 of b = field + bframe
};

// Uniform; mapped_plan over (keys, a), then b's eligibility for the walk.
__device__ __forceinline__ MappedProductPlan mapped_product_plan(const adac_segment_desc &kd, const MemberDomain &dom,
                                                                 const adac_segment_desc &ad, const adac_segment_desc &bd,
                                                                 const ProductTypes &ty) {
	MappedProductPlan p {mapped_plan<true>(kd, dom, ad, ty.a_tmask, ty.a_sbit), 0ull};
	if (p.m.p.reader == kMemWalk) {
		const bool walk = bd.width >= 1u && bd.width <= 32u && (uint64_t)bd.count * bd.width < (1ull << 31) &&
		                  product_frame(bd, ty.b_tmask, ty.b_sbit, p.bframe);
		if (!walk) p.m.p.reader = kMemStaged;
	}
	return p;
}

// The sink.  slice form: every row of the group whose t is in the domain has s0 <= t < s0 + 8 * nw.
template <bool A>
struct MappedProductBins {
	const uint8_t *map;        // d_map
	const uint8_t *slice;      // the LDS window
	unsigned long long *bab;   // the lane's copy of the LDS bins: SUM(a * b) ...
	unsigned long long *ba;    // ... SUM(a) (A) ...
	uint32_t *bcnt;            // ... and counts (when they are wanted)
	uint64_t s0;
	uint32_t ngroups;
	bool in_slice, cnt;        // uniform
	uint64_t osum_ab = 0;      // the overflow entry, in registers
	uint64_t osum_a = 0;
	uint32_t ocnt = 0;
	// a wanted row of index t < key_span and widened values va, vb
	__device__ __forceinline__ void row(uint64_t t, uint64_t va, uint64_t vb) {
		const uint32_t g = in_slice ? slice[(uint32_t)(t - s0)] : map[t];
		const uint64_t ab = va * vb;
		if (g < ngroups) {
			atomicAdd(&bab[g], (unsigned long long)ab);
			if (A) atomicAdd(&ba[g], (unsigned long long)va);
			if (cnt) atomicAdd(&bcnt[g], 1u);
		} else {
			osum_ab += ab;
			if (A) osum_a += va;
			ocnt++;
		}
	}
};

// Reader "walk": dense_key_walk with a second staged column.  Rows [r0, r1) of the segment triple, walked by ONE wave.
// `rows` gains the lane's wanted rows inside the domain.
template <int W, bool V, class Sink>
__device__ __forceinline__ void mapped_product_walk(uint32_t r0, uint32_t r1, const adac_segment_desc &kd,
                                                    const adac_segment_desc &ad, const adac_segment_desc &bd,
                                                    const uint4 *__restrict__ kseg16, const uint4 *__restrict__ aseg16,
                                                    const uint4 *__restrict__ bseg16,
                                                    const uint64_t *__restrict__ validity, uint4 *astage, uint4 *bstage,
                                                    const MappedProductPlan &plan, uint64_t key_span, Sink &sink,
                                                    uint32_t &rows) {
	constexpr int MAXV = ChunkWindow<W>::MAXV;
	const uint32_t wa = ad.width, amask = mask32(wa);
	const uint32_t wb = bd.width, bmask = mask32(wb);
	const uint32_t wmax = wa > wb ? wa : wb;
	// as many lanes as keep the round's rows of BOTH columns inside their buffers (product_walk's bound at the wider one)
	uint32_t lanes = ((kProdWaveData - 2u) * 128u) / ((uint32_t)MAXV * wmax);
	lanes = lanes < 64u ? lanes : 64u;
	const ChunkRange<W> run(r0, r1, kd.count);
	const uint32_t c0 = run.c0, c1 = run.c1;
	const uint32_t aclast = (uint32_t)(((uint64_t)ad.count * wa + 127) >> 7) - 1; // last chunk holding data bits of a
	const uint32_t bclast = (uint32_t)(((uint64_t)bd.count * wb + 127) >> 7) - 1; // ... of b
	const uint32_t lane = threadIdx.x & 63u;
	const bool walker = lane < lanes;
	uint32_t L = c0 + lane;
	uint4 q;
	uint32_t e;
	run.load(kseg16, L, q, e);
	const ChunkMask<W, V> vmask(validity, kd.val_off, r1); // the keys' element space
	uint64_t vm0 = 0, vm1 = 0;
	if (V) vmask.words(run.clamp(L), vm0, vm1);
	// a staged column of width w: s0 = its chunk holding the first bit of the round's first row, ns chunks in all (<= 128)
	auto round_s = [&](uint32_t rc, uint32_t w, uint32_t &s0, uint32_t &ns) {
		const uint32_t lo = chunk_first_row<W>(rc);
		uint32_t hi = chunk_first_row<W>(rc + lanes);
		hi = hi < r1 ? hi : r1;
		s0 = (lo * w) >> 7;
		ns = hi > lo ? ((hi * w + 127u) >> 7) - s0 : 0u;
	};
	// (two named chunks per column, not arrays of two: dense_key_walk records that as an array they went to scratch)
	auto load_s = [&](const uint4 *__restrict__ seg16, uint32_t s0, uint32_t slast, uint4 &v0, uint4 &v1) {
		const uint32_t c = s0 + lane; // unconditional, index clamped into the column's own segment
		v0 = seg16[c < slast ? c : slast];
		v1 = seg16[c + 64u < slast ? c + 64u : slast];
	};
	auto store_s = [&](uint4 *stage, const uint4 &v0, const uint4 &v1, uint32_t ns) { // lane (+ 64) < ns <= 128
		if (lane < ns) stage[lane] = v0;
		if (lane + 64u < ns) stage[lane + 64u] = v1;
	};
	const uint32_t *a32 = reinterpret_cast<const uint32_t *>(astage);
	const uint32_t *b32 = reinterpret_cast<const uint32_t *>(bstage);
	uint32_t ac0 = 0, na = 0, bc0 = 0, nb = 0;
	uint4 aq0, aq1, bq0, bq1;
	round_s(c0, wa, ac0, na);
	round_s(c0, wb, bc0, nb);
	load_s(aseg16, ac0, aclast, aq0, aq1);
	load_s(bseg16, bc0, bclast, bq0, bq1);
	store_s(astage, aq0, aq1, na);
	store_s(bstage, bq0, bq1, nb);
	for (uint32_t round0 = c0; round0 < c1; round0 += lanes, L += lanes) { // uniform trip count
		uint4 qn;
		uint32_t en;
		run.load(kseg16, L + lanes, qn, en);
		uint64_t vn0 = 0, vn1 = 0;
		if (V) vmask.words(run.clamp(L + lanes), vn0, vn1);
		uint32_t ac0n = 0, nan = 0, bc0n = 0, nbn = 0;
		round_s(round0 + lanes, wa, ac0n, nan);
		round_s(round0 + lanes, wb, bc0n, nbn);
		load_s(aseg16, ac0n, aclast, aq0, aq1);
		load_s(bseg16, bc0n, bclast, bq0, bq1);
		if (walker && L < c1) {
			const ChunkWindow<W> cw(q, e, L, r1);
			const uint32_t have = cw.have();
			// rows that exist AND are wanted, as one mask
			uint32_t vb = have >= 32u ? 0xffffffffu : ((1u << have) - 1u);
			if (V) vb &= (uint32_t)vmask.window(vm0, vm1, cw.i0 < r1 ? cw.i0 : r1);
			const uint32_t abit = cw.i0 * wa - 128u * ac0; // row i0 of a inside its staged chunks
			const uint32_t bbit = cw.i0 * wb - 128u * bc0; // ... of b
#pragma unroll
			for (int j = 0; j < MAXV; j++) {
				const uint64_t t = (uint64_t)field_of<W>(cw.nrm, j) + plan.m.p.delta;
				if (((vb >> j) & 1u) != 0u && t < key_span) {
					const uint64_t va = (uint64_t)staged_field32(a32, abit + (uint32_t)j * wa, amask) + plan.m.p.vframe;
					const uint64_t vbv = (uint64_t)staged_field32(b32, bbit + (uint32_t)j * wb, bmask) + plan.bframe;
					sink.row(t, va, vbv);
					rows++;
				}
			}
		}
		q = qn;
		e = en;
		vm0 = vn0;
		vm1 = vn1;
		store_s(astage, aq0, aq1, nan); // after this round's reads of the buffers
		store_s(bstage, bq0, bq1, nbn);
		ac0 = ac0n;
		bc0 = bc0n;
	}
}

struct MappedProductStage {
	const uint4 *ksrc, *asrc, *bsrc; // the 16-byte chunks holding the first bit of the rows
	uint32_t kbit0, abit0, bbit0, kchunks, achunks, bchunks, row0, m;
};

// Reader "staged": dense_key_staged_pair with a third column.  Every thread runs every barrier.
template <bool V, class Sink>
__device__ __forceinline__ uint32_t mapped_product_staged(const ScanGroup &g, const adac_segment_desc &ad,
                                                          const adac_segment_desc &bd,
                                                          const uint64_t *__restrict__ kwords,
                                                          const uint64_t *__restrict__ awords,
                                                          const uint64_t *__restrict__ bwords, const MemberDomain &dom,
                                                          const ProductTypes &ty, const uint64_t *__restrict__ validity,
                                                          uint4 *lds, Sink &sink) {
	uint4 *kstage[2] = {lds, lds + kCmpStageChunks};
	uint4 *astage[2] = {lds + 2 * kCmpStageChunks, lds + 3 * kCmpStageChunks};
	uint4 *bstage[2] = {lds + 4 * kCmpStageChunks, lds + 5 * kCmpStageChunks};
	const adac_segment_desc &kd = g.d;
	const uint32_t tid = threadIdx.x;
	const uint32_t wk = kd.width, wa = ad.width, wb = bd.width;
	uint32_t wmax = wk > wa ? wk : wa;
	wmax = wmax > wb ? wmax : wb;
	uint32_t per_stage = ((kCmpStageBytes * 8u - 256u) / (wmax ? wmax : 1u)) & ~(uint32_t)(kWorkgroup - 1);
	per_stage = per_stage < (uint32_t)kWorkgroup ? (uint32_t)kWorkgroup : per_stage;
	const uint4 *k16 = reinterpret_cast<const uint4 *>(kwords + kd.word_off);
	const uint4 *a16 = reinterpret_cast<const uint4 *>(awords + ad.word_off);
	const uint4 *b16 = reinterpret_cast<const uint4 *>(bwords + bd.word_off);
	const uint64_t kadd = effective_add(kd), aadd = effective_add(ad), badd = effective_add(bd);
	auto make_stage = [&](uint32_t done, MappedProductStage &st) -> bool {
		if (done >= g.n) return false;
		st.row0 = g.first + done;
		st.m = g.n - done < per_stage ? g.n - done : per_stage;
		const uint64_t kpos = (uint64_t)st.row0 * wk, apos = (uint64_t)st.row0 * wa, bpos = (uint64_t)st.row0 * wb;
		st.ksrc = k16 + (kpos >> 7);
		st.asrc = a16 + (apos >> 7);
		st.bsrc = b16 + (bpos >> 7);
		st.kbit0 = (uint32_t)(kpos & 127);
		st.abit0 = (uint32_t)(apos & 127);
		st.bbit0 = (uint32_t)(bpos & 127);
		st.kchunks = (st.kbit0 + st.m * wk + 127u) >> 7; // <= kCmpStageBytes / 16 + 1: one per thread
		st.achunks = (st.abit0 + st.m * wa + 127u) >> 7;
		st.bchunks = (st.bbit0 + st.m * wb + 127u) >> 7;
		return true;
	};
	MappedProductStage cur, nxt;
	uint32_t done = 0;
	bool have = make_stage(done, cur); // uniform
	uint4 kq, aq, bq;
	if (have) {
		if (tid < cur.kchunks) kstage[0][tid] = cur.ksrc[tid];
		if (tid < cur.achunks) astage[0][tid] = cur.asrc[tid];
		if (tid < cur.bchunks) bstage[0][tid] = cur.bsrc[tid];
	}
	__syncthreads();
	const uint32_t kmlo = wk >= 32u ? 0xffffffffu : mask32(wk), kmhi = wk > 32u ? mask32(wk - 32u) : 0u;
	const uint32_t amlo = wa >= 32u ? 0xffffffffu : mask32(wa), amhi = wa > 32u ? mask32(wa - 32u) : 0u;
	const uint32_t bmlo = wb >= 32u ? 0xffffffffu : mask32(wb), bmhi = wb > 32u ? mask32(wb - 32u) : 0u;
	uint32_t rows = 0;
	uint32_t buf = 0;
	while (have) { // uniform
		done += cur.m;
		const bool more = make_stage(done, nxt);
		if (more) { // in flight while this stage is consumed: unconditional loads, index clamped into the stage
			kq = nxt.ksrc[tid < nxt.kchunks ? tid : (nxt.kchunks ? nxt.kchunks - 1u : 0u)];
			aq = nxt.asrc[tid < nxt.achunks ? tid : (nxt.achunks ? nxt.achunks - 1u : 0u)];
			bq = nxt.bsrc[tid < nxt.bchunks ? tid : (nxt.bchunks ? nxt.bchunks - 1u : 0u)];
		}
		const uint32_t *k32 = reinterpret_cast<const uint32_t *>(kstage[buf]);
		const uint32_t *a32 = reinterpret_cast<const uint32_t *>(astage[buf]);
		const uint32_t *b32 = reinterpret_cast<const uint32_t *>(bstage[buf]);
		const uint64_t elem0 = kd.val_off + cur.row0; // the keys' element space
		for (uint32_t base = 0; base < cur.m; base += (uint32_t)kWorkgroup) { // uniform trip count
			const uint32_t row = base + tid;
			const uint32_t rr = row < cur.m ? row : cur.m - 1u; // clamped: the reads stay inside the stage and the mask
			const uint64_t fk = staged_field(k32, cur.kbit0 + rr * wk, kmlo, kmhi);
			const uint64_t fa = staged_field(a32, cur.abit0 + rr * wa, amlo, amhi);
			const uint64_t fb = staged_field(b32, cur.bbit0 + rr * wb, bmlo, bmhi);
			const uint32_t keep = V ? (validity_window_pair(validity, elem0 + rr, 1u) & 1u) : 1u;
			const uint64_t t = ((((fk + kadd) & dom.tmask) ^ dom.sbit) - dom.bbase);
			uint64_t x = (fa + aadd) & ty.a_tmask;
			x = (x ^ ty.a_sbit) - ty.a_sbit; // widened by a's signedness
			uint64_t y = (fb + badd) & ty.b_tmask;
			y = (y ^ ty.b_sbit) - ty.b_sbit; // ... by b's
			if (row < cur.m && keep != 0u && t < dom.set_bits) {
				sink.row(t, x, y);
				rows++;
			}
		}
		if (more) {
			if (tid < nxt.kchunks) kstage[buf ^ 1u][tid] = kq;
			if (tid < nxt.achunks) astage[buf ^ 1u][tid] = aq;
			if (tid < nxt.bchunks) bstage[buf ^ 1u][tid] = bq;
		}
		__syncthreads();
		cur = nxt;
		have = more;
		buf ^= 1u;
	}
	return rows;
}

// V: a mask is given; A: d_sums_a is wanted.  copies: a power of two with copies * ngroups <= kMappedProductBins
// (mapped_copies).
template <bool V, bool A>
__global__ __launch_bounds__(kWorkgroup, kMappedProductResident) void k_group_mapped_product(
    const ScanGroup *__restrict__ kgroups, const uint64_t *__restrict__ kwords,
    const adac_segment_desc *__restrict__ adescs, const uint64_t *__restrict__ awords,
    const adac_segment_desc *__restrict__ bdescs, const uint64_t *__restrict__ bwords, MemberDomain dom, ProductTypes ty,
    const uint64_t *__restrict__ validity, const uint8_t *__restrict__ map, uint32_t ngroups, uint32_t copies,
    unsigned long long *sums_ab, unsigned long long *sums_a, unsigned long long *counts,
    unsigned long long *__restrict__ seg_rows) {
	__shared__ uint4 lds[2 * kCmpLdsChunks]; // walk: a's four per-wave stages, then b's; staged: six buffers
	__shared__ unsigned long long slice[kMappedSliceWords];
	__shared__ unsigned long long bab[kMappedProductBins];
	__shared__ unsigned long long ba[A ? kMappedProductBins : 1];
	__shared__ uint32_t bcnt[kMappedProductBins];
	const ScanGroup g = load_scan_group(kgroups, blockIdx.x);
	const adac_segment_desc ad = load_desc_scalar(adescs, g.seg);
	const adac_segment_desc bd = load_desc_scalar(bdescs, g.seg);
	const MappedProductPlan plan = mapped_product_plan(g.d, dom, ad, bd, ty);
	const uint32_t reader = plan.m.p.reader;
	const bool live = reader != kMemHeader;  // uniform
	const bool cnt = counts != nullptr;      // uniform
	const uint32_t nbins = ngroups * copies; // <= kMappedProductBins
	if (live) {
		for (uint32_t i = threadIdx.x; i < nbins; i += (uint32_t)kWorkgroup) {
			bab[i] = 0ull;
			if (A) ba[i] = 0ull;
			bcnt[i] = 0u;
		}
		if (plan.m.slice) mapped_slice_fill(plan.m, map, dom.set_bits, slice);
	}
	__syncthreads();
	const uint32_t mine = (threadIdx.x & (copies - 1u)) * ngroups; // the lane's copy
	MappedProductBins<A> sink {map, reinterpret_cast<const uint8_t *>(slice), bab + mine, ba + (A ? mine : 0u), bcnt + mine,
	                           plan.m.s0, ngroups, plan.m.slice, cnt};
	uint32_t rows = 0;
	if (reader == kMemWalk) {
		const uint32_t wave = threadIdx.x >> 6;
		const RwQuarter qr(g, wave);
		if (!qr.empty()) { // uniform per wave; the walk has no barrier
			dispatch_width_4_32(g.d.width, [&](auto wc) __attribute__((always_inline)) {
				mapped_product_walk<decltype(wc)::value, V>(qr.r0, qr.r1, g.d, ad, bd,
				                                            reinterpret_cast<const uint4 *>(kwords + g.d.word_off),
				                                            reinterpret_cast<const uint4 *>(awords + ad.word_off),
				                                            reinterpret_cast<const uint4 *>(bwords + bd.word_off), validity,
				                                            lds + wave * kProdWaveChunks,
				                                            lds + kCmpLdsChunks + wave * kProdWaveChunks, plan,
				                                            dom.set_bits, sink, rows);
			});
		}
	} else if (reader == kMemStaged) {
		rows = mapped_product_staged<V>(g, ad, bd, kwords, awords, bwords, dom, ty, validity, lds, sink);
	}
	dense_key_seg_rows(seg_rows, g.seg, rows);
	// the overflow entry: one reduction per wave
	const uint64_t osum_ab = wave_sum(sink.osum_ab);
	const uint64_t osum_a = A ? wave_sum(sink.osum_a) : 0ull;
	const uint64_t ocnt = wave_sum((uint64_t)sink.ocnt);
	if ((threadIdx.x & 63u) == 0u && ocnt != 0ull) {
		if (osum_ab != 0ull) atomicAdd(sums_ab + ngroups, (unsigned long long)osum_ab);
		if (A && osum_a != 0ull) atomicAdd(sums_a + ngroups, (unsigned long long)osum_a);
		if (cnt) atomicAdd(counts + ngroups, (unsigned long long)ocnt);
	}
	__syncthreads(); // every wave's rows are in the bins
	if (live) {
		for (uint32_t b = threadIdx.x; b < ngroups; b += (uint32_t)kWorkgroup) {
			unsigned long long sab = 0ull, sa = 0ull;
			uint32_t c = 0u;
			for (uint32_t k = 0; k < copies; k++) {
				sab += bab[k * ngroups + b];
				if (A) sa += ba[k * ngroups + b];
				c += bcnt[k * ngroups + b];
			}
			if (sab) atomicAdd(sums_ab + b, sab);
			if (A && sa) atomicAdd(sums_a + b, sa);
			if (cnt && c) atomicAdd(counts + b, (unsigned long long)c);
		}
	}
}
