// adac_group_q1.inl — all of Q1's grouped sums in ONE scan: COUNT, SUM(q), SUM(a), SUM(b), SUM(a * b), SUM(a * c) and
// SUM(a * b * c) GROUP BY key over FIVE packed columns of the same table under a selection bitmap
// (adac_scan_group_sum_q1; Q1: a = price, b = discount, c = tax, q = quantity).  The six grouped calls it replaces read
// price, the keys and the mask once each: 146 packed bits per row at Q1's widths against 42 here.
// Included into adac_kernels.hip inside namespace adac::{anonymous}, after adac_group_product3.inl: the chunk walk
// (adac_chunk_walk.inl), product_frame (adac_sum_product.inl), the a / b / c / key part of the eligibility rule
// (group_product3_rw_eligible), the key reader RwKeys and the fast kernel's shell (adac_group_rw_walk.inl) and the stage
// structure (adac_group_sum.inl) are shared as they are; no existing kernel calls into this file.
//
// Semantics, term by term those of the calls it replaces: each value is widened to 64 bits by its own column's
// signedness, products and sums are taken mod 2^64; key = the key column's value as an unsigned number of its own
// width, rows whose key >= ngroups land in bin `ngroups`; a row whose bit is clear in the mask — indexed in a's element
// space, val_off + row — is added to no term of no bin.  Nothing is materialised.
//
// Two forms, chosen per scan group of `a` by group_q1_rw_eligible — uniform, a function of the five descriptors, the
// five types and ngroups alone, so both kernels (and the host mirror, bench_configs.group_q1_form_groups) agree:
//   fast     (k_group_q1_rw)  group_product3_rw_eligible(a, b, c, keys) AND the same for q as for c: linear (or raw and
//            unsigned), 1 <= wq <= 32, below 2^31 bits, 0 <= frame and frame + 2^wq - 1 <= 2^32 - 1.  So all four values
//            are unsigned 32-bit numbers for EVERY field of the segment.  group_product3_walk's structure with a third
//            staged
//            column: `a` on the width-templated register walk, the chunks of b, c AND q that hold the round's rows each
//            staged in a wave-private LDS buffer (requested a round ahead, stored after the round's reads: no barrier
//            in the loop), keys through RwKeys (DIRECT or staged bytes).  Lanes per round: group_product3_walk's bound
//            at the widest
//            of wb, wc and wq.  A row costs x, y, z, v as 32-bit numbers, x, y and v ANDed with the row's 0 / -1 mask
//            (masking x alone would leave SUM(b), SUM(q) and COUNT standing; z meets x only), the exact x y and x z, (x y) z as
//            product3 makes it, and six ds_add_u64 + one ds_add_u32 without return.
//   generic  (k_group_q1)     everything else: widths 1..64, all eight types in every role, raw and unpacked segments,
//            ADAC_NO_MIN, the all-ones stored min, nbins > 8, segments of 2^31 bits and more.  k_group_product3's
//            structure with a fifth staged column and seven bin arrays.
// Bins: per wave kGroupQ1RwCopies copies of 8 bins of six 64-bit sums and one 32-bit count, in LDS (a copy's count is
// the rows of one bin that its four lanes met in one launch: far below 2^32, as in k_group_product3_rw).
// Finishing: one partial row of 7 x nbins words per workgroup in a's partial buffer (shared with the other grouped
// scans, as are the hand-over words and the call counter), k_group_q1_final adds them into d_out[t * nbins + bin].

constexpr uint32_t kGroupQ1Terms = 7; // ADAC_Q1_COUNT, SUM_Q, SUM_A, SUM_B, SUM_AB, SUM_AC, SUM_ABC: the header's order

struct GroupQ1Types {
	GroupProduct3Types g; // a, b, c and the key type, a's tile rows
	uint64_t q_tmask, q_sbit;
};

struct GroupQ1Plan {
	GroupProduct3Plan g; // ok, ma, mb, mc, the key side
	uint32_t mq;         // value = field + frame, as an unsigned 32-bit number
};

// Can the register-walk kernel take this segment quintuple?  (The file header states the rule.)
__device__ __forceinline__ GroupQ1Plan group_q1_rw_eligible(const adac_segment_desc &ad, const adac_segment_desc &bd,
                                                            const adac_segment_desc &cd, const adac_segment_desc &qd,
                                                            const adac_segment_desc &kd, const GroupQ1Types &ty,
                                                            uint32_t ngroups) {
	GroupQ1Plan p;
	p.g = group_product3_rw_eligible(ad, bd, cd, kd, ty.g, ngroups);
	p.mq = 0u;
	if (!p.g.g.ok) return p;
	p.g.g.ok = false;
	const uint32_t wq = qd.width;
	if (wq < 1u || wq > 32u || (uint64_t)qd.count * wq >= (1ull << 31)) return p;
	uint64_t mq = 0ull;
	if (!product_frame(qd, ty.q_tmask, ty.q_sbit, mq)) return p;
	if (mq > 0xffffffffull - mask64(wq)) return p; // a frame below zero is a huge unsigned number and fails the same test
	p.mq = (uint32_t)mq;
	p.g.g.ok = true;
	return p;
}

// ------------------------------------------------------------------------------------------------------------------
// generic form
// ------------------------------------------------------------------------------------------------------------------
struct GroupQ1Stage {
	const uint4 *asrc, *bsrc, *csrc, *qsrc, *ksrc; // the 16-byte chunks holding the first bit of the rows
	uint64_t aadd, badd, cadd, qadd, kadd;
	uint32_t abit0, bbit0, cbit0, qbit0, kbit0, achunks, bchunks, cchunks, qchunks, kchunks, wa, wb, wc, wq, wk, m;
};

// bin sets per wave of the generic kernel (lane & 7 picks one).  Half of kGroupCopies: six 64-bit bin arrays at 16 sets
// would be 24 KiB next to 36 KiB of stage buffers, two workgroups per CU; at 8 sets the workgroup needs about 51 KiB and
// three are resident.  NOT measured against 16 sets at two residents: the generic form is the exception path.
constexpr uint32_t kGroupQ1Copies = 8;
// workgroups per CU the generic kernel's grid is sized from: 5 x 2 stage buffers + mask words + seven bin arrays
constexpr uint32_t kGroupQ1Resident = 3;

template <bool V>
__global__ __launch_bounds__(kWorkgroup) void k_group_q1(
    const adac_segment_desc *__restrict__ adescs, const TileRef *__restrict__ atiles, uint32_t ntiles,
    const uint64_t *__restrict__ awords, const adac_segment_desc *__restrict__ bdescs,
    const uint64_t *__restrict__ bwords, const adac_segment_desc *__restrict__ cdescs,
    const uint64_t *__restrict__ cwords, const adac_segment_desc *__restrict__ qdescs,
    const uint64_t *__restrict__ qwords, const adac_segment_desc *__restrict__ kdescs,
    const uint64_t *__restrict__ kwords, GroupQ1Types ty, uint32_t ngroups, unsigned long long *__restrict__ partial,
    const unsigned long long *__restrict__ rw_fallback, const uint64_t *__restrict__ validity) {
	// Runs after k_group_q1_rw (when that kernel was launched: rw_fallback != nullptr) and takes what it left
	if (rw_fallback != nullptr && *rw_fallback == 0ull) return; // uniform (the final kernel then leaves these partials out)
	const bool skip_rw = rw_fallback != nullptr;
	__shared__ uint4 astage[2][kGroupStageBytes / 16 + 2];
	__shared__ uint4 bstage[2][kGroupStageBytes / 16 + 2];
	__shared__ uint4 cstage[2][kGroupStageBytes / 16 + 2];
	__shared__ uint4 qstage[2][kGroupStageBytes / 16 + 2];
	__shared__ uint4 kstage[2][kGroupStageBytes / 16 + 2];
	__shared__ uint64_t mstage[2][V ? kGroupMaskWords + 1 : 1];
	constexpr uint32_t kSets = (kWorkgroup / 64) * kGroupQ1Copies;
	constexpr uint32_t kBinSlots = kGroupPrivateBins * kSets > kGroupMaxBins ? kGroupPrivateBins * kSets : kGroupMaxBins;
	constexpr uint32_t kSums = kGroupQ1Terms - 1u; // the six 64-bit terms; COUNT is 32 bits per slot
	__shared__ unsigned long long bsum[kSums][kBinSlots];
	__shared__ uint32_t bcnt[kBinSlots];
	const uint32_t my_set = (threadIdx.x >> 6) * kGroupQ1Copies + (threadIdx.x & (kGroupQ1Copies - 1u));
	const uint32_t nbins = ngroups + 1u;
	const bool priv = nbins <= kGroupPrivateBins; // uniform
	const uint32_t tid = threadIdx.x;
	for (uint32_t i = tid; i < kBinSlots; i += kWorkgroup) {
#pragma unroll
		for (uint32_t t = 0; t < kSums; t++) bsum[t][i] = 0ull;
		bcnt[i] = 0u;
	}
	// tiles blockIdx.x, + gridDim.x, ... of a's layout; the tile reference is fetched two tiles ahead and the five
	// descriptors one tile ahead (k_group_sum)
	struct TileMeta {
		TileRef r;
		adac_segment_desc ad, bd, cd, qd, kd;
		bool valid;
		bool taken; // by k_group_q1_rw
	};
	const uint32_t G = gridDim.x;
	auto fetch_ref = [&](uint32_t tile) { return atiles[tile < ntiles ? tile : 0u]; };
	auto resolve = [&](TileRef r, uint32_t tile) {
		TileMeta m;
		m.r = r;
		m.ad = load_desc_scalar(adescs, r.seg);
		m.bd = load_desc_scalar(bdescs, r.seg);
		m.cd = load_desc_scalar(cdescs, r.seg);
		m.qd = load_desc_scalar(qdescs, r.seg);
		m.kd = load_desc_scalar(kdescs, r.seg);
		m.valid = tile < ntiles;
		m.taken = skip_rw && m.valid && group_q1_rw_eligible(m.ad, m.bd, m.cd, m.qd, m.kd, ty, ngroups).g.g.ok;
		return m;
	};
	uint32_t t = blockIdx.x, done = 0;
	TileMeta mcur = resolve(fetch_ref(t), t);
	TileMeta mnxt = resolve(fetch_ref(t + G), t + G);
	TileRef rnn = fetch_ref(t + 2u * G);
	auto advance = [&]() {
		mcur = mnxt;
		t += G;
		mnxt = resolve(rnn, t + G);
		rnn = fetch_ref(t + 2u * G);
		done = 0;
	};
	using StageMask = std::conditional_t<V, GroupStageMask, GroupStageNoMask>;
	const uint32_t a_tile_rows = ty.g.g.a_tile_rows;
	auto next_stage = [&](GroupQ1Stage &g, StageMask &gm) -> bool {
		if (mcur.valid) {
			const uint32_t left = mcur.ad.count - mcur.r.first;
			const uint32_t n = left < a_tile_rows ? left : a_tile_rows;
			if (done >= n) advance(); // uniform: on to the next tile
		}
		while (mcur.valid && mcur.taken) advance(); // uniform
		if (!mcur.valid) return false;
		const uint32_t left = mcur.ad.count - mcur.r.first;
		const uint32_t n = left < a_tile_rows ? left : a_tile_rows;
		g.wa = mcur.ad.width;
		g.wb = mcur.bd.width;
		g.wc = mcur.cd.width;
		g.wq = mcur.qd.width;
		g.wk = mcur.kd.width;
		uint32_t wmax = g.wa > g.wb ? g.wa : g.wb;
		wmax = wmax > g.wc ? wmax : g.wc;
		wmax = wmax > g.wq ? wmax : g.wq;
		wmax = wmax > g.wk ? wmax : g.wk; // >= 1: no segment has width 0
		uint32_t per_stage = ((kGroupStageBytes * 8u - 256u) / wmax) & ~(uint32_t)(kWorkgroup - 1);
		per_stage = per_stage < (uint32_t)kWorkgroup ? (uint32_t)kWorkgroup : per_stage;
		per_stage = per_stage < kGroupMaskStageRows ? per_stage : kGroupMaskStageRows; // also unmasked, as in k_group_product3: widths 1 - 3 then take the same stages in either form
		g.m = n - done < per_stage ? n - done : per_stage;
		if constexpr (V) { // element index of the stage's first row, in 64 bits: val_off alone may exceed 2^32
			const uint64_t e0 = mcur.ad.val_off + (uint64_t)(mcur.r.first + done);
			gm.src = validity + (e0 >> 6);
			gm.sh = (uint32_t)(e0 & 63u);
			gm.words = (gm.sh + g.m + 63u) >> 6; // g.m >= 1: 1 .. kGroupMaskWords words, each holds the bit of a row
		}
		const uint64_t row = (uint64_t)(mcur.r.first + done);
		const uint64_t apos = row * g.wa, bpos = row * g.wb, cpos = row * g.wc, qpos = row * g.wq, kpos = row * g.wk;
		g.asrc = reinterpret_cast<const uint4 *>(awords + mcur.ad.word_off) + (apos >> 7);
		g.bsrc = reinterpret_cast<const uint4 *>(bwords + mcur.bd.word_off) + (bpos >> 7);
		g.csrc = reinterpret_cast<const uint4 *>(cwords + mcur.cd.word_off) + (cpos >> 7);
		g.qsrc = reinterpret_cast<const uint4 *>(qwords + mcur.qd.word_off) + (qpos >> 7);
		g.ksrc = reinterpret_cast<const uint4 *>(kwords + mcur.kd.word_off) + (kpos >> 7);
		g.abit0 = (uint32_t)(apos & 127);
		g.bbit0 = (uint32_t)(bpos & 127);
		g.cbit0 = (uint32_t)(cpos & 127);
		g.qbit0 = (uint32_t)(qpos & 127);
		g.kbit0 = (uint32_t)(kpos & 127);
		g.achunks = (g.abit0 + g.m * g.wa + 127u) >> 7; // <= kGroupStageBytes / 16 + 1 <= two per thread, >= 1
		g.bchunks = (g.bbit0 + g.m * g.wb + 127u) >> 7;
		g.cchunks = (g.cbit0 + g.m * g.wc + 127u) >> 7;
		g.qchunks = (g.qbit0 + g.m * g.wq + 127u) >> 7;
		g.kchunks = (g.kbit0 + g.m * g.wk + 127u) >> 7;
		g.aadd = effective_add(mcur.ad);
		g.badd = effective_add(mcur.bd);
		g.cadd = effective_add(mcur.cd);
		g.qadd = effective_add(mcur.qd);
		g.kadd = effective_add(mcur.kd);
		done += g.m;
		return true;
	};
	GroupQ1Stage cur, nxt;
	StageMask mk_cur, mk_nxt;
	bool have = next_stage(cur, mk_cur); // uniform
	uint4 aq[kGroupChunksPerThread], bq[kGroupChunksPerThread], cq[kGroupChunksPerThread], qq[kGroupChunksPerThread],
	    kq[kGroupChunksPerThread];
	uint64_t mq = 0;
	if (have) {
#pragma unroll
		for (uint32_t h = 0; h < kGroupChunksPerThread; h++) { // chunks <= kGroupStageBytes / 16 + 1: inside the buffer
			const uint32_t c = tid + h * kWorkgroup;
			if (c < cur.achunks) astage[0][c] = cur.asrc[c];
			if (c < cur.bchunks) bstage[0][c] = cur.bsrc[c];
			if (c < cur.cchunks) cstage[0][c] = cur.csrc[c];
			if (c < cur.qchunks) qstage[0][c] = cur.qsrc[c];
			if (c < cur.kchunks) kstage[0][c] = cur.ksrc[c];
		}
		if constexpr (V) {
			if (tid < mk_cur.words) mstage[0][tid] = mk_cur.src[tid];
		}
	}
	__syncthreads();
	uint32_t buf = 0;
	while (have) {
		const bool more = next_stage(nxt, mk_nxt);
		if (more) { // in flight while this stage is aggregated: unconditional loads, index clamped into the stage
#pragma unroll
			for (uint32_t h = 0; h < kGroupChunksPerThread; h++) {
				const uint32_t c = tid + h * kWorkgroup;
				aq[h] = nxt.asrc[c < nxt.achunks ? c : nxt.achunks - 1u];
				bq[h] = nxt.bsrc[c < nxt.bchunks ? c : nxt.bchunks - 1u];
				cq[h] = nxt.csrc[c < nxt.cchunks ? c : nxt.cchunks - 1u];
				qq[h] = nxt.qsrc[c < nxt.qchunks ? c : nxt.qchunks - 1u];
				kq[h] = nxt.ksrc[c < nxt.kchunks ? c : nxt.kchunks - 1u];
			}
			if constexpr (V) mq = mk_nxt.src[tid < mk_nxt.words ? tid : mk_nxt.words - 1u]; // clamped: no word outside the stage's rows
		}
		const uint32_t *a32 = reinterpret_cast<const uint32_t *>(astage[buf]);
		const uint32_t *b32 = reinterpret_cast<const uint32_t *>(bstage[buf]);
		const uint32_t *c32 = reinterpret_cast<const uint32_t *>(cstage[buf]);
		const uint32_t *q32 = reinterpret_cast<const uint32_t *>(qstage[buf]);
		const uint32_t *k32 = reinterpret_cast<const uint32_t *>(kstage[buf]);
		const uint32_t *m32 = reinterpret_cast<const uint32_t *>(mstage[buf]);
		auto kept = [&](uint32_t r) -> uint32_t { // row r's bit is bit sh + r of the staged words
			if constexpr (V) {
				const uint32_t b = mk_cur.sh + r;
				return (m32[b >> 5] >> (b & 31u)) & 1u;
			} else {
				return 1u;
			}
		};
		const uint32_t amlo = cur.wa >= 32u ? 0xffffffffu : mask32(cur.wa), amhi = cur.wa > 32u ? mask32(cur.wa - 32u) : 0u;
		const uint32_t bmlo = cur.wb >= 32u ? 0xffffffffu : mask32(cur.wb), bmhi = cur.wb > 32u ? mask32(cur.wb - 32u) : 0u;
		const uint32_t cmlo = cur.wc >= 32u ? 0xffffffffu : mask32(cur.wc), cmhi = cur.wc > 32u ? mask32(cur.wc - 32u) : 0u;
		const uint32_t qmlo = cur.wq >= 32u ? 0xffffffffu : mask32(cur.wq), qmhi = cur.wq > 32u ? mask32(cur.wq - 32u) : 0u;
		const uint32_t kmlo = cur.wk >= 32u ? 0xffffffffu : mask32(cur.wk), kmhi = cur.wk > 32u ? mask32(cur.wk - 32u) : 0u;
		// two rows per thread and round: the field reads are issued together, then the LDS adds
		for (uint32_t row0 = tid; row0 < cur.m; row0 += 2u * kWorkgroup) {
			uint64_t fa[2], fb[2], fc[2], fq[2], key[2];
			[[maybe_unused]] uint32_t keep[2];
#pragma unroll
			for (int u = 0; u < 2; u++) {
				const uint32_t row = row0 + (uint32_t)u * kWorkgroup;
				const uint32_t rr = row < cur.m ? row : row0; // clamped: the read stays inside the stage
				fa[u] = staged_field(a32, cur.abit0 + rr * cur.wa, amlo, amhi);
				fb[u] = staged_field(b32, cur.bbit0 + rr * cur.wb, bmlo, bmhi);
				fc[u] = staged_field(c32, cur.cbit0 + rr * cur.wc, cmlo, cmhi);
				fq[u] = staged_field(q32, cur.qbit0 + rr * cur.wq, qmlo, qmhi);
				key[u] = staged_field(k32, cur.kbit0 + rr * cur.wk, kmlo, kmhi);
				if constexpr (V) keep[u] = kept(rr);
			}
#pragma unroll
			for (int u = 0; u < 2; u++) {
				const uint32_t row = row0 + (uint32_t)u * kWorkgroup;
				uint64_t x = (fa[u] + cur.aadd) & ty.g.g.p.a_tmask;
				x = (x ^ ty.g.g.p.a_sbit) - ty.g.g.p.a_sbit; // widened by a's signedness
				uint64_t y = (fb[u] + cur.badd) & ty.g.g.p.b_tmask;
				y = (y ^ ty.g.g.p.b_sbit) - ty.g.g.p.b_sbit;
				uint64_t z = (fc[u] + cur.cadd) & ty.g.c_tmask;
				z = (z ^ ty.g.c_sbit) - ty.g.c_sbit;
				uint64_t v = (fq[u] + cur.qadd) & ty.q_tmask;
				v = (v ^ ty.q_sbit) - ty.q_sbit;
				const uint64_t k = (key[u] + cur.kadd) & ty.g.g.k_tmask;
				const uint32_t bin = k < (uint64_t)ngroups ? (uint32_t)k : ngroups;
				const uint32_t slot = priv ? bin * kSets + my_set : bin;
				if (row < cur.m && (!V || keep[u])) { // ds_add without return: nothing waits for them
					const uint64_t xy = x * y;
					atomicAdd(&bcnt[slot], 1u);
					atomicAdd(&bsum[0][slot], (unsigned long long)v);
					atomicAdd(&bsum[1][slot], (unsigned long long)x);
					atomicAdd(&bsum[2][slot], (unsigned long long)y);
					atomicAdd(&bsum[3][slot], (unsigned long long)xy);
					atomicAdd(&bsum[4][slot], (unsigned long long)(x * z));
					atomicAdd(&bsum[5][slot], (unsigned long long)(xy * z));
				}
			}
		}
		if (more) {
#pragma unroll
			for (uint32_t h = 0; h < kGroupChunksPerThread; h++) {
				const uint32_t c = tid + h * kWorkgroup;
				if (c < nxt.achunks) astage[buf ^ 1u][c] = aq[h];
				if (c < nxt.bchunks) bstage[buf ^ 1u][c] = bq[h];
				if (c < nxt.cchunks) cstage[buf ^ 1u][c] = cq[h];
				if (c < nxt.qchunks) qstage[buf ^ 1u][c] = qq[h];
				if (c < nxt.kchunks) kstage[buf ^ 1u][c] = kq[h];
			}
			if constexpr (V) {
				if (tid < mk_nxt.words) mstage[buf ^ 1u][tid] = mq;
			}
		}
		__syncthreads();
		cur = nxt;
		mk_cur = mk_nxt;
		have = more;
		buf ^= 1u;
	}
	// one partial row per workgroup: term t of bin b at [t * nbins + b]
	unsigned long long *__restrict__ mine = partial + (uint64_t)blockIdx.x * kGroupQ1Terms * nbins;
	if (priv) { // a bin's sets are added by one wave; the (term, bin) pairs go round the waves
		static_assert(kSets <= 64u, "one lane per bin set");
		const uint32_t wave = tid >> 6, lane = tid & 63u;
		for (uint32_t i = wave; i < kGroupQ1Terms * nbins; i += kWorkgroup / 64) { // uniform per wave
			const uint32_t term = i / nbins, b = i - term * nbins;
			uint64_t v = 0ull;
			if (lane < kSets) v = term == 0u ? (uint64_t)bcnt[b * kSets + lane] : (uint64_t)bsum[term - 1u][b * kSets + lane];
			v = wave_sum(v);
			if (lane == 0u) mine[i] = v;
		}
	} else {
		for (uint32_t i = tid; i < kGroupQ1Terms * nbins; i += kWorkgroup) {
			const uint32_t term = i / nbins, b = i - term * nbins;
			mine[i] = term == 0u ? (unsigned long long)bcnt[b] : bsum[term - 1u][b];
		}
	}
}

// ------------------------------------------------------------------------------------------------------------------
// fast form
// ------------------------------------------------------------------------------------------------------------------
// bin sets per wave of the fast kernel (lane & 15 picks one: four lanes share a set) and the workgroups per CU (= waves
// per SIMD) it is compiled for and its grid is sized from.  Seven terms at product3's 32 sets would be 52 KiB of bins per
// workgroup next to 28 KiB of stage buffers and 4 KiB of key bytes: one workgroup per CU.  At 16 sets the workgroup needs
// 58 KiB and two are resident in a CU's 160 KiB, with 256 VGPRs each: the third staged column (its two prefetched chunks,
// its fields and addressing) fits without spills, which it would not at four waves per SIMD (product3 sits at 113 of 128
// there).  Measured against 8 sets at three residents (22 % slower) and 32 at one (45 % slower): DESIGN.md §7, with what was not tried.
constexpr uint32_t kGroupQ1RwCopies = 16;
constexpr uint32_t kGroupQ1RwResident = 2;

// One QUARTER of a scan group, rows [r0, r1) (r0 a multiple of 128 rows: its bits start a chunk of `a`), walked by ONE
// wave: group_product3_walk with a third staged column and seven terms.  `keys`: the wave's kGroupRwWaveKeyBytes of key
// bytes (staged form), `bstage` / `cstage` / `qstage`: its kProdWaveChunks chunks of b, c and q, `wsum`: its six arrays
// of kGroupPrivateBins x kGroupQ1RwCopies 64-bit words (SUM_Q, SUM_A, SUM_B, SUM_AB, SUM_AC, SUM_ABC, kSlots apart),
// `wcnt`: its count words, all carried across the quarters the wave walks.
template <int W, bool DIRECT, bool V>
__device__ __forceinline__ void group_q1_walk(uint32_t r0, uint32_t r1, const adac_segment_desc &ad,
                                              const adac_segment_desc &bd, const adac_segment_desc &cd,
                                              const adac_segment_desc &qd, const GroupQ1Plan &plan,
                                              const uint4 *__restrict__ aseg16, const uint4 *__restrict__ bseg16,
                                              const uint4 *__restrict__ cseg16, const uint4 *__restrict__ qseg16,
                                              const RwKeyStream &ks, uint32_t ngroups,
                                              uint8_t *keys, uint4 *bstage, uint4 *cstage, uint4 *qstage,
                                              unsigned long long *wsum, uint32_t *wcnt,
                                              const uint64_t *__restrict__ validity) {
	constexpr int MAXV = ChunkWindow<W>::MAXV;
	constexpr int BATCH = 4;               // rows whose fields of b, c and q are read together (3 x BATCH LDS reads in flight)
	constexpr uint32_t kSlots = kGroupPrivateBins * kGroupQ1RwCopies;
	const GroupProductPlan &kp = plan.g.g;
	const uint32_t wb = bd.width, bmask = mask32(wb);
	const uint32_t wc = cd.width, cmask = mask32(wc);
	const uint32_t wq = qd.width, qmask = mask32(wq);
	uint32_t wmax = wb > wc ? wb : wc;
	wmax = wmax > wq ? wmax : wq;
	uint32_t lanes = ((kProdWaveData - 2u) * 128u) / ((uint32_t)MAXV * wmax); // >= 15: MAXV <= 32, wmax <= 32
	lanes = lanes < RwKeys<W, DIRECT>::LANES ? lanes : RwKeys<W, DIRECT>::LANES;
	const ChunkRange<W> run(r0, r1, ad.count);
	const uint32_t c0 = run.c0, c1 = run.c1;
	const uint32_t bclast = (uint32_t)(((uint64_t)bd.count * wb + 127) >> 7) - 1; // last chunk holding data bits of b
	const uint32_t cclast = (uint32_t)(((uint64_t)cd.count * wc + 127) >> 7) - 1; // ... of c
	const uint32_t qclast = (uint32_t)(((uint64_t)qd.count * wq + 127) >> 7) - 1; // ... of q
	const uint32_t lane = threadIdx.x & 63u;
	const bool walker = lane < lanes;
	unsigned long long *const my_sum = wsum + (lane & (kGroupQ1RwCopies - 1u));
	uint32_t *const my_cnt = wcnt + (lane & (kGroupQ1RwCopies - 1u));
	uint32_t L = c0 + lane;
	uint4 q;
	uint32_t e;
	run.load(aseg16, L, q, e);
	const ChunkMask<W, V> vmask(validity, ad.val_off, r1); // a's element space
	uint64_t vm0 = 0, vm1 = 0;
	if (V) vmask.words(run.clamp(L), vm0, vm1);
	// the rows of the round that starts at chunk rc of a: [first row starting in chunk rc, first row starting in chunk
	// rc + lanes) below r1
	// a staged column of width w: s0 = its chunk holding the first bit of the first of them, ns chunks in all (<= 128)
	auto round_s = [&](uint32_t rc, uint32_t w, uint32_t &s0, uint32_t &ns) {
		const uint32_t lo = chunk_first_row<W>(rc);
		uint32_t hi = chunk_first_row<W>(rc + lanes);
		hi = hi < r1 ? hi : r1;
		s0 = (lo * w) >> 7;
		ns = hi > lo ? ((hi * w + 127u) >> 7) - s0 : 0u;
	};
	// (two named chunks per lane and column, not an array: nothing here is indexed before the loops are unrolled)
	auto load_s = [&](const uint4 *__restrict__ seg16, uint32_t s0, uint32_t slast, uint4 &s_lo, uint4 &s_hi) { // unconditional, index clamped into the segment
		const uint32_t c = s0 + lane;
		s_lo = seg16[c < slast ? c : slast];
		s_hi = seg16[c + 64u < slast ? c + 64u : slast];
	};
	auto store_s = [&](uint4 *stage, const uint4 &s_lo, const uint4 &s_hi, uint32_t ns) { // lane + 64 p < ns <= 128: inside the buffer
		if (lane < ns) stage[lane] = s_lo;
		if (lane + 64u < ns) stage[lane + 64u] = s_hi;
	};
	const uint32_t *b32 = reinterpret_cast<const uint32_t *>(bstage);
	const uint32_t *c32 = reinterpret_cast<const uint32_t *>(cstage);
	const uint32_t *q32 = reinterpret_cast<const uint32_t *>(qstage);
	uint32_t bc0 = 0, nb = 0, cc0 = 0, nc = 0, qc0 = 0, nq = 0;
	uint4 bq0, bq1, cq0, cq1, qq0, qq1;
	round_s(c0, wb, bc0, nb);
	round_s(c0, wc, cc0, nc);
	round_s(c0, wq, qc0, nq);
	load_s(bseg16, bc0, bclast, bq0, bq1);
	load_s(cseg16, cc0, cclast, cq0, cq1);
	load_s(qseg16, qc0, qclast, qq0, qq1);
	store_s(bstage, bq0, bq1, nb);
	store_s(cstage, cq0, cq1, nc);
	store_s(qstage, qq0, qq1, nq);
	RwKeys<W, DIRECT> k(ks, kp.kadd_byte, kp.keys_overflow, keys, r1, lanes);
	k.first(c0, run.clamp(L));
	for (uint32_t round0 = c0; round0 < c1; round0 += lanes, L += lanes) { // uniform trip count
		// requested before this round is walked: the next chunk of a, its mask words, the next round's chunks of b, c, q and keys
		uint4 qn;
		uint32_t en;
		run.load(aseg16, L + lanes, qn, en);
		uint64_t vn0 = 0, vn1 = 0;
		if (V) vmask.words(run.clamp(L + lanes), vn0, vn1);
		uint32_t bc0n = 0, nbn = 0, cc0n = 0, ncn = 0, qc0n = 0, nqn = 0;
		round_s(round0 + lanes, wb, bc0n, nbn);
		round_s(round0 + lanes, wc, cc0n, ncn);
		round_s(round0 + lanes, wq, qc0n, nqn);
		load_s(bseg16, bc0n, bclast, bq0, bq1);
		load_s(cseg16, cc0n, cclast, cq0, cq1);
		load_s(qseg16, qc0n, qclast, qq0, qq1);
		k.request(round0 + lanes, run.clamp(L + lanes));
		if (walker && L < c1) {
			const ChunkWindow<W> cw(q, e, L, r1);
			const uint32_t have = cw.have();
			// rows that exist AND are kept, as one mask: the rows past the quarter's end add zero like the masked ones
			uint32_t vb = have >= 32u ? 0xffffffffu : ((1u << have) - 1u);
			if (V) vb &= (uint32_t)vmask.window(vm0, vm1, cw.i0 < r1 ? cw.i0 : r1);
			const uint32_t bbit = cw.i0 * wb - 128u * bc0; // row i0 of b inside its staged chunks
			const uint32_t cbit = cw.i0 * wc - 128u * cc0; // ... of c
			const uint32_t qbit = cw.i0 * wq - 128u * qc0; // ... of q
			uint32_t kwin, kn[RwKeys<W, DIRECT>::KD]; // DIRECT: the keys of rows i0 .. from bit 0; staged: their bytes
			k.window(cw.i0, kwin, kn);
			// BATCH rows at a time: their fields of b, c and q are read together, then consumed
#pragma unroll
			for (int j0 = 0; j0 < MAXV; j0 += BATCH) {
				uint32_t fb[BATCH], fc[BATCH], fq[BATCH];
#pragma unroll
				for (int u = 0; u < BATCH; u++) {
					if (j0 + u < MAXV) {
						fb[u] = staged_field32(b32, bbit + (uint32_t)(j0 + u) * wb, bmask);
						fc[u] = staged_field32(c32, cbit + (uint32_t)(j0 + u) * wc, cmask);
						fq[u] = staged_field32(q32, qbit + (uint32_t)(j0 + u) * wq, qmask);
					}
				}
#pragma unroll
				for (int u = 0; u < BATCH; u++) {
					if (j0 + u < MAXV) {
						const int j = j0 + u;
						const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)vb, (uint32_t)j, 1u); // 0 / -1
						const uint32_t bin = k.bin(kwin, kn, j, ngroups);
						// a masked row (or one past the run): every term adds zero, so x, y and v carry the mask (z meets x only)
						const uint32_t x = (field_of<W>(cw.nrm, j) + kp.ma) & m;
						const uint32_t y = (fb[u] + kp.mb) & m;
						const uint32_t z = fc[u] + plan.g.mc;
						const uint32_t v = (fq[u] + plan.mq) & m;
						const uint64_t xy = (uint64_t)x * y; // exact 32 x 32 -> 64
						const uint64_t xz = (uint64_t)x * z;
						const uint64_t xyz = (uint64_t)(uint32_t)xy * z + ((uint64_t)((uint32_t)(xy >> 32) * z) << 32); // mod 2^64
						unsigned long long *const s = my_sum + bin * kGroupQ1RwCopies;
						atomicAdd(my_cnt + bin * kGroupQ1RwCopies, m & 1u); // ds_add without return, all seven
						atomicAdd(s, (unsigned long long)v);
						atomicAdd(s + kSlots, (unsigned long long)x);
						atomicAdd(s + 2u * kSlots, (unsigned long long)y);
						atomicAdd(s + 3u * kSlots, (unsigned long long)xy);
						atomicAdd(s + 4u * kSlots, (unsigned long long)xz);
						atomicAdd(s + 5u * kSlots, (unsigned long long)xyz);
					}
				}
			}
		}
		q = qn;
		e = en;
		vm0 = vn0;
		vm1 = vn1;
		store_s(bstage, bq0, bq1, nbn); // after this round's reads of the buffers (LDS operations of one wave execute in order)
		store_s(cstage, cq0, cq1, ncn);
		store_s(qstage, qq0, qq1, nqn);
		bc0 = bc0n;
		cc0 = cc0n;
		qc0 = qc0n;
		k.commit();
	}
}

template <bool V>
__global__ __launch_bounds__(kWorkgroup, kGroupQ1RwResident) void k_group_q1_rw(
    const ScanGroup *__restrict__ agroups, uint32_t ngroups_work, const uint64_t *__restrict__ awords,
    const adac_segment_desc *__restrict__ bdescs, const uint64_t *__restrict__ bwords,
    const adac_segment_desc *__restrict__ cdescs, const uint64_t *__restrict__ cwords,
    const adac_segment_desc *__restrict__ qdescs, const uint64_t *__restrict__ qwords,
    const adac_segment_desc *__restrict__ kdescs, const uint64_t *__restrict__ kwords, GroupQ1Types ty, uint32_t ngroups,
    unsigned long long *__restrict__ partial, unsigned long long *__restrict__ fallback,
    const uint64_t *__restrict__ validity) {
	constexpr uint32_t kWaves = kWorkgroup / 64;
	constexpr uint32_t kSlots = kGroupPrivateBins * kGroupQ1RwCopies; // bin words per wave and term
	constexpr uint32_t kSums = kGroupQ1Terms - 1u;
	__shared__ __attribute__((aligned(16))) uint8_t keys[kWaves][kGroupRwWaveKeyBytes];
	__shared__ uint4 bstage[kWaves][kProdWaveChunks];
	__shared__ uint4 cstage[kWaves][kProdWaveChunks];
	__shared__ uint4 qstage[kWaves][kProdWaveChunks];
	__shared__ unsigned long long sums[kWaves][kSums * kSlots];
	__shared__ uint32_t cnts[kWaves][kSlots];
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
	const uint32_t nbins = ngroups + 1u;
	for (uint32_t i = lane; i < kSums * kSlots; i += 64u) sums[wave][i] = 0ull;
	for (uint32_t i = lane; i < kSlots; i += 64u) cnts[wave][i] = 0u;
	uint32_t skipped = 0;
	for (uint32_t gi = blockIdx.x; gi < ngroups_work; gi += gridDim.x) {
		const ScanGroup g = load_scan_group(agroups, gi);
		const adac_segment_desc bd = load_desc(bdescs + g.seg);
		const adac_segment_desc cd = load_desc(cdescs + g.seg);
		const adac_segment_desc qd = load_desc(qdescs + g.seg);
		const adac_segment_desc kd = load_desc(kdescs + g.seg);
		const GroupQ1Plan plan = group_q1_rw_eligible(g.d, bd, cd, qd, kd, ty, ngroups);
		if (!plan.g.g.ok) { // uniform
			skipped++;
			continue;
		}
		const RwQuarter qr(g, wave);
		if (qr.empty()) continue; // uniform per wave
		const uint4 *aseg16 = reinterpret_cast<const uint4 *>(awords + g.d.word_off);
		const uint4 *bseg16 = reinterpret_cast<const uint4 *>(bwords + bd.word_off);
		const uint4 *cseg16 = reinterpret_cast<const uint4 *>(cwords + cd.word_off);
		const uint4 *qseg16 = reinterpret_cast<const uint4 *>(qwords + qd.word_off);
		const RwKeyStream ks(kwords, kd);
		group_rw_dispatch(g.d.width, ks.direct(g.d.width), [&](auto wt, auto direct) __attribute__((always_inline)) {
			group_q1_walk<decltype(wt)::value, decltype(direct)::value, V>(
			    qr.r0, qr.r1, g.d, bd, cd, qd, plan, aseg16, bseg16, cseg16, qseg16, ks, ngroups,
			    keys[wave], bstage[wave], cstage[wave], qstage[wave], sums[wave], cnts[wave], validity);
		});
	}
	if (skipped && tid == 0u) atomicAdd(fallback, (unsigned long long)skipped);
	// the wave's own total per (term, bin): its kGroupQ1RwCopies copies added by one lane each (7 x nbins <= 56 lanes;
	// the wave's own words: LDS operations of one wave execute in order), then the four waves' totals through LDS
	__shared__ unsigned long long tot[kWaves][kGroupQ1Terms * kGroupPrivateBins];
	if (lane < kGroupQ1Terms * nbins) {
		const uint32_t term = lane / nbins, b = lane - term * nbins;
		unsigned long long s = 0ull;
		if (term == 0u) {
#pragma unroll
			for (uint32_t c = 0; c < kGroupQ1RwCopies; c++) s += cnts[wave][b * kGroupQ1RwCopies + c];
		} else {
#pragma unroll
			for (uint32_t c = 0; c < kGroupQ1RwCopies; c++) s += sums[wave][(term - 1u) * kSlots + b * kGroupQ1RwCopies + c];
		}
		tot[wave][lane] = s;
	}
	__syncthreads();
	// one partial row per workgroup: term t of bin b at [t * nbins + b]
	unsigned long long *__restrict__ mine = partial + (uint64_t)blockIdx.x * kGroupQ1Terms * nbins;
	if (tid < kGroupQ1Terms * nbins) {
		unsigned long long v = 0ull;
#pragma unroll
		for (uint32_t w = 0; w < kWaves; w++) v += tot[w][tid];
		mine[tid] = v;
	}
}

// one workgroup per bin: the partial rows of all workgroups -> out[t * nbins + bin] for the seven terms.  The rows of
// k_group_q1 are read only when it had something to do (no register-walk kernel, or *rw_fallback != 0).
__global__ __launch_bounds__(kWorkgroup) void k_group_q1_final(const unsigned long long *__restrict__ partial,
                                                               uint32_t nwg_rw, uint32_t nwg_staged, uint32_t nbins,
                                                               uint64_t *__restrict__ out,
                                                               const unsigned long long *__restrict__ rw_fallback,
                                                               unsigned long long *__restrict__ next_fallback, int rw_ran) {
	__shared__ uint64_t ps[kWorkgroup / 64][kGroupQ1Terms];
	const uint32_t b = blockIdx.x;
	// the hand-over word alternates between two slots from call to call: this call's is still being read by the other
	// workgroups of this kernel, so the one the NEXT call will use is cleared here (k_group_final)
	if (b == 0u && threadIdx.x == 0u) *next_fallback = 0ull;
	const bool staged_ran = !rw_ran || *rw_fallback != 0ull; // uniform
	const uint32_t nwg = nwg_rw + (staged_ran ? nwg_staged : 0u);
	uint64_t s[kGroupQ1Terms];
#pragma unroll
	for (uint32_t t = 0; t < kGroupQ1Terms; t++) s[t] = 0ull;
	for (uint32_t g = threadIdx.x; g < nwg; g += kWorkgroup) {
#pragma unroll
		for (uint32_t t = 0; t < kGroupQ1Terms; t++) s[t] += partial[((uint64_t)g * kGroupQ1Terms + t) * nbins + b];
	}
#pragma unroll
	for (uint32_t t = 0; t < kGroupQ1Terms; t++) {
		const uint64_t v = wave_sum(s[t]);
		if ((threadIdx.x & 63u) == 0u) ps[threadIdx.x >> 6][t] = v;
	}
	__syncthreads();
	if (threadIdx.x < kGroupQ1Terms) {
		uint64_t v = 0ull;
#pragma unroll
		for (int w = 0; w < kWorkgroup / 64; w++) v += ps[w][threadIdx.x];
		out[(uint64_t)threadIdx.x * nbins + b] = v;
	}
}
