// adac_group_product3.inl — Q1's last aggregate: SUM(a * b * c) GROUP BY key over FOUR packed columns of the same table
// under a selection bitmap.  With integer decimals
//   sum_charge = SUM(p (100 - d)(100 + t)) = 10000 SUM(p) + 100 SUM(p t) - 100 SUM(p d) - SUM(p d t)   per group:
// the first term is adac_scan_group_sum_valid's, the next two are adac_scan_group_sum_product's, the fourth is this
// file's.  Included into adac_kernels.hip inside namespace adac::{anonymous}, after adac_group_product.inl: the chunk
// walk (adac_chunk_walk.inl), product_frame (adac_sum_product.inl), the a / b / key part of the eligibility rule
// (group_product_rw_eligible), the key reader RwKeys and the fast kernel's shell (adac_group_rw_walk.inl), the bin geometry
// and the stage structure (adac_group_sum.inl) are shared;
// no existing kernel calls into this file.
//
// Semantics: adac_scan_group_sum_product's with one more factor.  Each value is widened to 64 bits by its own column's
// signedness, both multiplications and the sums are taken mod 2^64; key = the key column's value as an unsigned number
// of its own width, rows whose key >= ngroups land in bin `ngroups`; a row whose bit is clear in the mask — indexed in
// a's element space, val_off + row — is added to no bin.  Nothing is materialised.
//
// Two forms, chosen per scan group of `a` by group_product3_rw_eligible — uniform, a function of the four descriptors,
// the four types and ngroups alone, so both kernels (and the host mirror, bench_configs.group_product3_form_groups)
// agree on who takes what:
//   fast     (k_group_product3_rw)  ALL of
//              * group_product_rw_eligible(a, b, keys): nbins = ngroups + 1 <= 8; a and b linear (or raw and unsigned),
//                4 <= wa <= 32, 1 <= wb <= 32, both below 2^31 bits, frame + 2^w - 1 <= 2^32 - 1 with a frame >= 0 on
//                either side; wk <= 8, keys that do not wrap in their type and either all fit a byte or all are
//                >= ngroups;
//              * the same for c as for b: linear (or raw and unsigned), 1 <= wc <= 32, below 2^31 bits,
//                0 <= frame and frame + 2^wc - 1 <= 2^32 - 1.
//            So all three widened values are unsigned 32-bit numbers for EVERY field of the segment.  (Q1: price at
//            frame + 24 bits, discount 0..10 in 4 bits, tax 0..8 in 4 bits, six groups in 3 bits: fast.)
//            group_product_walk's structure with a second staged column: `a` on the width-templated register walk,
//            the chunks of
//            b AND of c that hold the round's rows each staged in a wave-private LDS buffer (requested a round ahead,
//            stored after the round's reads: no barrier in the loop), keys through RwKeys: DIRECT or staged
//            bytes.  Lanes per round: as many as keep the round's key rows inside the key bytes and its rows of BOTH
//            staged columns inside their buffers — the bound of group_product_walk taken at the wider of wb and wc.
//            A row costs x = (fa + ma) & m, y = fb + mb, z = fc + mc as 32-bit numbers, the exact 64-bit x y, then
//            (x y) z mod 2^64 = lo(x y) z + ((hi(x y) z) << 32): three 32-bit multiplies, and ONE ds_add_u64 without
//            return (+ one ds_add_u32 when counts are wanted: template parameter C).  A masked row adds zero.
//   generic  (k_group_product3)     everything else: widths 1..64, all eight types on every side, raw and unpacked
//            segments, ADAC_NO_MIN, the all-ones stored min, frames that wrap a signed type, nbins > 8, segments of
//            2^31 bits and more.  k_group_product's structure with a fourth staged column; value =
//            (((field + effective_add) & tmask) ^ sbit) - sbit per column, two 64-bit multiplies.  Bit positions are
//            64-bit.
// Residency: the fast kernel is compiled for and launched on kGroupProduct3RwResident workgroups per CU, the generic one
// sized from kGroupProduct3Resident (the constants say why).  Finishing as in launch_group_product: hand-over word,
// partial buffer, call counter are the `a` layout's, shared with the other grouped scans; k_group_final adds the
// partials.

struct GroupProduct3Types {
	GroupProductTypes g;      // a, b and the key type, a's tile rows
	uint64_t c_tmask, c_sbit; // c: all-ones mask of the type's width, its sign bit
};

struct GroupProduct3Plan {
	GroupProductPlan g; // ok, ma, mb, the key side
	uint32_t mc;        // value = field + frame, as an unsigned 32-bit number
};

// Can the register-walk kernel take this segment quadruple?  (The file header states the rule.)
__device__ __forceinline__ GroupProduct3Plan group_product3_rw_eligible(const adac_segment_desc &ad,
                                                                        const adac_segment_desc &bd,
                                                                        const adac_segment_desc &cd,
                                                                        const adac_segment_desc &kd,
                                                                        const GroupProduct3Types &ty, uint32_t ngroups) {
	GroupProduct3Plan p;
	p.g = group_product_rw_eligible(ad, bd, kd, ty.g, ngroups);
	p.mc = 0u;
	if (!p.g.ok) return p;
	p.g.ok = false;
	const uint32_t wc = cd.width;
	if (wc < 1u || wc > 32u || (uint64_t)cd.count * wc >= (1ull << 31)) return p;
	uint64_t mc = 0ull;
	if (!product_frame(cd, ty.c_tmask, ty.c_sbit, mc)) return p;
	if (mc > 0xffffffffull - mask64(wc)) return p; // a frame below zero is a huge unsigned number and fails the same test
	p.mc = (uint32_t)mc;
	p.g.ok = true;
	return p;
}

// ------------------------------------------------------------------------------------------------------------------
// generic form
// ------------------------------------------------------------------------------------------------------------------
struct GroupProduct3Stage {
	const uint4 *asrc, *bsrc, *csrc, *ksrc; // the 16-byte chunks holding the first bit of the rows
	uint64_t aadd, badd, cadd, kadd;
	uint32_t abit0, bbit0, cbit0, kbit0, achunks, bchunks, cchunks, kchunks, wa, wb, wc, wk, m;
};

// workgroups per CU the generic kernel's grid is sized from: 4 x 2 stage buffers + mask words + bins = 37 KiB of LDS
constexpr uint32_t kGroupProduct3Resident = 4;

template <bool V>
__global__ __launch_bounds__(kWorkgroup) void k_group_product3(
    const adac_segment_desc *__restrict__ adescs, const TileRef *__restrict__ atiles, uint32_t ntiles,
    const uint64_t *__restrict__ awords, const adac_segment_desc *__restrict__ bdescs,
    const uint64_t *__restrict__ bwords, const adac_segment_desc *__restrict__ cdescs,
    const uint64_t *__restrict__ cwords, const adac_segment_desc *__restrict__ kdescs,
    const uint64_t *__restrict__ kwords, GroupProduct3Types ty, uint32_t ngroups,
    unsigned long long *__restrict__ partial, const unsigned long long *__restrict__ rw_fallback,
    const uint64_t *__restrict__ validity) {
	// Runs after k_group_product3_rw (when that kernel was launched: rw_fallback != nullptr) and takes what it left
	if (rw_fallback != nullptr && *rw_fallback == 0ull) return; // uniform (the final kernel then leaves these partials out)
	const bool skip_rw = rw_fallback != nullptr;
	__shared__ uint4 astage[2][kGroupStageBytes / 16 + 2];
	__shared__ uint4 bstage[2][kGroupStageBytes / 16 + 2];
	__shared__ uint4 cstage[2][kGroupStageBytes / 16 + 2];
	__shared__ uint4 kstage[2][kGroupStageBytes / 16 + 2];
	__shared__ uint64_t mstage[2][V ? kGroupMaskWords + 1 : 1];
	constexpr uint32_t kSets = (kWorkgroup / 64) * kGroupCopies;
	constexpr uint32_t kBinSlots = kGroupPrivateBins * kSets > kGroupMaxBins ? kGroupPrivateBins * kSets : kGroupMaxBins;
	__shared__ unsigned long long bsum[kBinSlots];
	__shared__ uint32_t bcnt[kBinSlots];
	const uint32_t my_set = (threadIdx.x >> 6) * kGroupCopies + (threadIdx.x & (kGroupCopies - 1u));
	const uint32_t nbins = ngroups + 1u;
	const bool priv = nbins <= kGroupPrivateBins; // uniform
	const uint32_t tid = threadIdx.x;
	for (uint32_t i = tid; i < kBinSlots; i += kWorkgroup) {
		bsum[i] = 0ull;
		bcnt[i] = 0u;
	}
	// tiles blockIdx.x, + gridDim.x, ... of a's layout; the tile reference is fetched two tiles ahead and the four
	// descriptors one tile ahead (k_group_sum)
	struct TileMeta {
		TileRef r;
		adac_segment_desc ad, bd, cd, kd;
		bool valid;
		bool taken; // by k_group_product3_rw
	};
	const uint32_t G = gridDim.x;
	auto fetch_ref = [&](uint32_t tile) { return atiles[tile < ntiles ? tile : 0u]; };
	auto resolve = [&](TileRef r, uint32_t tile) {
		TileMeta m;
		m.r = r;
		m.ad = load_desc_scalar(adescs, r.seg);
		m.bd = load_desc_scalar(bdescs, r.seg);
		m.cd = load_desc_scalar(cdescs, r.seg);
		m.kd = load_desc_scalar(kdescs, r.seg);
		m.valid = tile < ntiles;
		m.taken = skip_rw && m.valid && group_product3_rw_eligible(m.ad, m.bd, m.cd, m.kd, ty, ngroups).g.ok;
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
	const uint32_t a_tile_rows = ty.g.a_tile_rows;
	auto next_stage = [&](GroupProduct3Stage &g, StageMask &gm) -> bool {
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
		g.wk = mcur.kd.width;
		uint32_t wmax = g.wa > g.wb ? g.wa : g.wb;
		wmax = wmax > g.wc ? wmax : g.wc;
		wmax = wmax > g.wk ? wmax : g.wk; // >= 1: no segment has width 0
		uint32_t per_stage = ((kGroupStageBytes * 8u - 256u) / wmax) & ~(uint32_t)(kWorkgroup - 1);
		per_stage = per_stage < (uint32_t)kWorkgroup ? (uint32_t)kWorkgroup : per_stage;
		per_stage = per_stage < kGroupMaskStageRows ? per_stage : kGroupMaskStageRows;
		g.m = n - done < per_stage ? n - done : per_stage;
		if constexpr (V) { // element index of the stage's first row, in 64 bits: val_off alone may exceed 2^32
			const uint64_t e0 = mcur.ad.val_off + (uint64_t)(mcur.r.first + done);
			gm.src = validity + (e0 >> 6);
			gm.sh = (uint32_t)(e0 & 63u);
			gm.words = (gm.sh + g.m + 63u) >> 6; // g.m >= 1: 1 .. kGroupMaskWords words, each holds the bit of a row
		}
		const uint64_t row = (uint64_t)(mcur.r.first + done);
		const uint64_t apos = row * g.wa, bpos = row * g.wb, cpos = row * g.wc, kpos = row * g.wk;
		g.asrc = reinterpret_cast<const uint4 *>(awords + mcur.ad.word_off) + (apos >> 7);
		g.bsrc = reinterpret_cast<const uint4 *>(bwords + mcur.bd.word_off) + (bpos >> 7);
		g.csrc = reinterpret_cast<const uint4 *>(cwords + mcur.cd.word_off) + (cpos >> 7);
		g.ksrc = reinterpret_cast<const uint4 *>(kwords + mcur.kd.word_off) + (kpos >> 7);
		g.abit0 = (uint32_t)(apos & 127);
		g.bbit0 = (uint32_t)(bpos & 127);
		g.cbit0 = (uint32_t)(cpos & 127);
		g.kbit0 = (uint32_t)(kpos & 127);
		g.achunks = (g.abit0 + g.m * g.wa + 127u) >> 7; // <= kGroupStageBytes / 16 + 1 <= two per thread, >= 1
		g.bchunks = (g.bbit0 + g.m * g.wb + 127u) >> 7;
		g.cchunks = (g.cbit0 + g.m * g.wc + 127u) >> 7;
		g.kchunks = (g.kbit0 + g.m * g.wk + 127u) >> 7;
		g.aadd = effective_add(mcur.ad);
		g.badd = effective_add(mcur.bd);
		g.cadd = effective_add(mcur.cd);
		g.kadd = effective_add(mcur.kd);
		done += g.m;
		return true;
	};
	GroupProduct3Stage cur, nxt;
	StageMask mk_cur, mk_nxt;
	bool have = next_stage(cur, mk_cur); // uniform
	uint4 aq[kGroupChunksPerThread], bq[kGroupChunksPerThread], cq[kGroupChunksPerThread], kq[kGroupChunksPerThread];
	uint64_t mq = 0;
	if (have) {
#pragma unroll
		for (uint32_t h = 0; h < kGroupChunksPerThread; h++) { // chunks <= kGroupStageBytes / 16 + 1: inside the buffer
			const uint32_t c = tid + h * kWorkgroup;
			if (c < cur.achunks) astage[0][c] = cur.asrc[c];
			if (c < cur.bchunks) bstage[0][c] = cur.bsrc[c];
			if (c < cur.cchunks) cstage[0][c] = cur.csrc[c];
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
				kq[h] = nxt.ksrc[c < nxt.kchunks ? c : nxt.kchunks - 1u];
			}
			if constexpr (V) mq = mk_nxt.src[tid < mk_nxt.words ? tid : mk_nxt.words - 1u]; // clamped: no word outside the stage's rows
		}
		const uint32_t *a32 = reinterpret_cast<const uint32_t *>(astage[buf]);
		const uint32_t *b32 = reinterpret_cast<const uint32_t *>(bstage[buf]);
		const uint32_t *c32 = reinterpret_cast<const uint32_t *>(cstage[buf]);
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
		const uint32_t kmlo = cur.wk >= 32u ? 0xffffffffu : mask32(cur.wk), kmhi = cur.wk > 32u ? mask32(cur.wk - 32u) : 0u;
		// four rows per thread and round: the field reads are issued together, then the LDS adds
		for (uint32_t row0 = tid; row0 < cur.m; row0 += 4u * kWorkgroup) {
			uint64_t fa[4], fb[4], fc[4], key[4];
			[[maybe_unused]] uint32_t keep[4];
#pragma unroll
			for (int u = 0; u < 4; u++) {
				const uint32_t row = row0 + (uint32_t)u * kWorkgroup;
				const uint32_t rr = row < cur.m ? row : row0; // clamped: the read stays inside the stage
				fa[u] = staged_field(a32, cur.abit0 + rr * cur.wa, amlo, amhi);
				fb[u] = staged_field(b32, cur.bbit0 + rr * cur.wb, bmlo, bmhi);
				fc[u] = staged_field(c32, cur.cbit0 + rr * cur.wc, cmlo, cmhi);
				key[u] = staged_field(k32, cur.kbit0 + rr * cur.wk, kmlo, kmhi);
				if constexpr (V) keep[u] = kept(rr);
			}
#pragma unroll
			for (int u = 0; u < 4; u++) {
				const uint32_t row = row0 + (uint32_t)u * kWorkgroup;
				uint64_t x = (fa[u] + cur.aadd) & ty.g.p.a_tmask;
				x = (x ^ ty.g.p.a_sbit) - ty.g.p.a_sbit; // widened by a's signedness
				uint64_t y = (fb[u] + cur.badd) & ty.g.p.b_tmask;
				y = (y ^ ty.g.p.b_sbit) - ty.g.p.b_sbit;
				uint64_t z = (fc[u] + cur.cadd) & ty.c_tmask;
				z = (z ^ ty.c_sbit) - ty.c_sbit;
				const uint64_t k = (key[u] + cur.kadd) & ty.g.k_tmask;
				const uint32_t bin = k < (uint64_t)ngroups ? (uint32_t)k : ngroups;
				const uint32_t slot = priv ? bin * kSets + my_set : bin;
				if (row < cur.m && (!V || keep[u])) {
					atomicAdd(&bsum[slot], (unsigned long long)(x * y * z)); // ds_add_u64, no return: nothing waits for it
					atomicAdd(&bcnt[slot], 1u);
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
	// one partial per bin and workgroup
	unsigned long long *__restrict__ mine = partial + (uint64_t)blockIdx.x * 2u * nbins;
	if (priv) { // a bin's sets are added by the first wave
		if (tid < 64u) {
			for (uint32_t b = 0; b < nbins; b++) { // uniform
				static_assert(kSets <= 64u, "one lane per bin set");
				const uint64_t sv = tid < kSets ? (uint64_t)bsum[b * kSets + tid] : 0ull;
				const uint64_t cv = tid < kSets ? (uint64_t)bcnt[b * kSets + tid] : 0ull;
				const uint64_t ssum = wave_sum(sv), csum = wave_sum(cv);
				if (tid == 0u) {
					mine[2u * b] = ssum;
					mine[2u * b + 1u] = csum;
				}
			}
		}
	} else {
		for (uint32_t b = tid; b < nbins; b += kWorkgroup) {
			mine[2u * b] = bsum[b];
			mine[2u * b + 1u] = (unsigned long long)bcnt[b];
		}
	}
}

// ------------------------------------------------------------------------------------------------------------------
// fast form
// ------------------------------------------------------------------------------------------------------------------
// One QUARTER of a scan group, rows [r0, r1) (r0 a multiple of 128 rows: its bits start a chunk of `a`), walked by ONE
// wave: group_product_walk with a second staged column.  `keys`: the wave's kGroupRwWaveKeyBytes of key bytes (staged
// form), `bstage` / `cstage`: its kProdWaveChunks chunks of b and of c, `wsum` / `wcnt`: its kGroupPrivateBins x
// kGroupRwCopies bin words, carried across the quarters the wave walks.
// Lanes per round: as many as keep the round's key rows inside `keys` (RwKeys::LANES) AND its rows of b inside
// `bstage` AND its rows of c inside `cstage`: product_walk's bound at wmax = the wider of wb and wc (rows <= lanes *
// MAXV, so the bits of either column are <= 126 chunks, which from any bit offset of the first chunk lie in 128).
template <int W, bool DIRECT, bool V, bool C>
__device__ __forceinline__ void group_product3_walk(uint32_t r0, uint32_t r1, const adac_segment_desc &ad,
                                                    const adac_segment_desc &bd, const adac_segment_desc &cd,
                                                    const GroupProduct3Plan &plan,
                                                    const uint4 *__restrict__ aseg16, const uint4 *__restrict__ bseg16,
                                                    const uint4 *__restrict__ cseg16, const RwKeyStream &ks,
                                                    uint32_t ngroups, uint8_t *keys, uint4 *bstage,
                                                    uint4 *cstage, unsigned long long *wsum, uint32_t *wcnt,
                                                    const uint64_t *__restrict__ validity) {
	constexpr int MAXV = ChunkWindow<W>::MAXV;
	constexpr int BATCH = 4;               // rows whose fields of b and c are read together (2 x BATCH LDS reads in flight)
	const uint32_t wb = bd.width, bmask = mask32(wb);
	const uint32_t wc = cd.width, cmask = mask32(wc);
	const uint32_t wmax = wb > wc ? wb : wc;
	uint32_t lanes = ((kProdWaveData - 2u) * 128u) / ((uint32_t)MAXV * wmax); // >= 15: MAXV <= 32, wmax <= 32
	lanes = lanes < RwKeys<W, DIRECT>::LANES ? lanes : RwKeys<W, DIRECT>::LANES;
	const ChunkRange<W> run(r0, r1, ad.count);
	const uint32_t c0 = run.c0, c1 = run.c1;
	const uint32_t bclast = (uint32_t)(((uint64_t)bd.count * wb + 127) >> 7) - 1; // last chunk holding data bits of b
	const uint32_t cclast = (uint32_t)(((uint64_t)cd.count * wc + 127) >> 7) - 1; // ... of c
	const uint32_t lane = threadIdx.x & 63u;
	const bool walker = lane < lanes;
	unsigned long long *const my_sum = wsum + (lane & (kGroupRwCopies - 1u));
	uint32_t *const my_cnt = wcnt + (lane & (kGroupRwCopies - 1u));
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
	auto load_s = [&](const uint4 *__restrict__ seg16, uint32_t s0, uint32_t slast, uint4 (&sq)[2]) { // unconditional, index clamped into the segment
#pragma unroll
		for (uint32_t p = 0; p < 2; p++) {
			const uint32_t c = s0 + lane + 64u * p;
			sq[p] = seg16[c < slast ? c : slast];
		}
	};
	auto store_s = [&](uint4 *stage, const uint4 (&sq)[2], uint32_t ns) { // lane + 64 p < ns <= 128: inside the buffer
#pragma unroll
		for (uint32_t p = 0; p < 2; p++) {
			if (lane + 64u * p < ns) stage[lane + 64u * p] = sq[p];
		}
	};
	const uint32_t *b32 = reinterpret_cast<const uint32_t *>(bstage);
	const uint32_t *c32 = reinterpret_cast<const uint32_t *>(cstage);
	uint32_t bc0 = 0, nb = 0, cc0 = 0, nc = 0;
	uint4 bq[2], cq[2];
	round_s(c0, wb, bc0, nb);
	round_s(c0, wc, cc0, nc);
	load_s(bseg16, bc0, bclast, bq);
	load_s(cseg16, cc0, cclast, cq);
	store_s(bstage, bq, nb);
	store_s(cstage, cq, nc);
	RwKeys<W, DIRECT> k(ks, plan.g.kadd_byte, plan.g.keys_overflow, keys, r1, lanes);
	k.first(c0, run.clamp(L));
	for (uint32_t round0 = c0; round0 < c1; round0 += lanes, L += lanes) { // uniform trip count
		// requested before this round is walked: the next chunk of a, its mask words, the next round's chunks of b, c and keys
		uint4 qn;
		uint32_t en;
		run.load(aseg16, L + lanes, qn, en);
		uint64_t vn0 = 0, vn1 = 0;
		if (V) vmask.words(run.clamp(L + lanes), vn0, vn1);
		uint32_t bc0n = 0, nbn = 0, cc0n = 0, ncn = 0;
		round_s(round0 + lanes, wb, bc0n, nbn);
		round_s(round0 + lanes, wc, cc0n, ncn);
		load_s(bseg16, bc0n, bclast, bq);
		load_s(cseg16, cc0n, cclast, cq);
		k.request(round0 + lanes, run.clamp(L + lanes));
		if (walker && L < c1) {
			const ChunkWindow<W> cw(q, e, L, r1);
			const uint32_t have = cw.have();
			// rows that exist AND are kept, as one mask: the rows past the quarter's end add zero like the masked ones
			uint32_t vb = have >= 32u ? 0xffffffffu : ((1u << have) - 1u);
			if (V) vb &= (uint32_t)vmask.window(vm0, vm1, cw.i0 < r1 ? cw.i0 : r1);
			const uint32_t bbit = cw.i0 * wb - 128u * bc0; // row i0 of b inside its staged chunks
			const uint32_t cbit = cw.i0 * wc - 128u * cc0; // ... of c
			uint32_t kwin, kn[RwKeys<W, DIRECT>::KD]; // DIRECT: the keys of rows i0 .. from bit 0; staged: their bytes
			k.window(cw.i0, kwin, kn);
			// BATCH rows at a time: their fields of b and c are read together, then consumed
#pragma unroll
			for (int j0 = 0; j0 < MAXV; j0 += BATCH) {
				uint32_t fb[BATCH], fc[BATCH];
#pragma unroll
				for (int u = 0; u < BATCH; u++) {
					if (j0 + u < MAXV) {
						fb[u] = staged_field32(b32, bbit + (uint32_t)(j0 + u) * wb, bmask);
						fc[u] = staged_field32(c32, cbit + (uint32_t)(j0 + u) * wc, cmask);
					}
				}
#pragma unroll
				for (int u = 0; u < BATCH; u++) {
					if (j0 + u < MAXV) {
						const int j = j0 + u;
						const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)vb, (uint32_t)j, 1u); // 0 / -1
						const uint32_t bin = k.bin(kwin, kn, j, ngroups);
						const uint32_t x = (field_of<W>(cw.nrm, j) + plan.g.ma) & m; // a masked row: 0 x y z = 0
						const uint32_t y = fb[u] + plan.g.mb;
						const uint32_t z = fc[u] + plan.mc;
						const uint64_t xy = (uint64_t)x * y;                                       // exact 32 x 32 -> 64
						const uint64_t xyz = (uint64_t)(uint32_t)xy * z + ((uint64_t)((uint32_t)(xy >> 32) * z) << 32); // mod 2^64
						atomicAdd(my_sum + bin * kGroupRwCopies, (unsigned long long)xyz); // ds_add_u64, no return
						if (C) atomicAdd(my_cnt + bin * kGroupRwCopies, m & 1u);
					}
				}
			}
		}
		q = qn;
		e = en;
		vm0 = vn0;
		vm1 = vn1;
		k.commit(); // before the columns' stores (after them the unmasked kernels spill one SGPR more: DESIGN.md §7)
		store_s(bstage, bq, nbn); // after this round's reads of the buffers (LDS operations of one wave execute in order)
		store_s(cstage, cq, ncn);
		bc0 = bc0n;
		cc0 = cc0n;
	}
}

// workgroups per CU (= waves per SIMD) the fast kernel is compiled for and its grid is sized from.  k_group_product_rw
// sits at 101 - 109 VGPRs of the 128 that four waves per SIMD allow; the second staged column adds its two prefetched
// chunks, its fields and its addressing on top.  Its LDS (keys + two stages + bins, about 35 KiB per workgroup) fits four
// workgroups in a CU's 160 KiB as well.
constexpr uint32_t kGroupProduct3RwResident = 4;

template <bool V, bool C>
__global__ __launch_bounds__(kWorkgroup, kGroupProduct3RwResident) void k_group_product3_rw(
    const ScanGroup *__restrict__ agroups, uint32_t ngroups_work, const uint64_t *__restrict__ awords,
    const adac_segment_desc *__restrict__ bdescs, const uint64_t *__restrict__ bwords,
    const adac_segment_desc *__restrict__ cdescs, const uint64_t *__restrict__ cwords,
    const adac_segment_desc *__restrict__ kdescs, const uint64_t *__restrict__ kwords, GroupProduct3Types ty,
    uint32_t ngroups, unsigned long long *__restrict__ partial, unsigned long long *__restrict__ fallback,
    const uint64_t *__restrict__ validity) {
	constexpr uint32_t kWaves = kWorkgroup / 64;
	constexpr uint32_t kSlots = kGroupPrivateBins * kGroupRwCopies; // bin words per wave
	__shared__ __attribute__((aligned(16))) uint8_t keys[kWaves][kGroupRwWaveKeyBytes];
	__shared__ uint4 bstage[kWaves][kProdWaveChunks];
	__shared__ uint4 cstage[kWaves][kProdWaveChunks];
	__shared__ unsigned long long sums[kWaves * kSlots];
	__shared__ uint32_t cnts[C ? kWaves * kSlots : 1];
	__shared__ unsigned long long red[2][2 * kGroupPrivateBins];
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
	const uint32_t nbins = ngroups + 1u;
	for (uint32_t i = lane; i < kSlots; i += 64u) {
		sums[wave * kSlots + i] = 0ull;
		if (C) cnts[wave * kSlots + i] = 0u;
	}
	uint32_t skipped = 0;
	for (uint32_t gi = blockIdx.x; gi < ngroups_work; gi += gridDim.x) {
		const ScanGroup g = load_scan_group(agroups, gi);
		const adac_segment_desc bd = load_desc(bdescs + g.seg);
		const adac_segment_desc cd = load_desc(cdescs + g.seg);
		const adac_segment_desc kd = load_desc(kdescs + g.seg);
		const GroupProduct3Plan plan = group_product3_rw_eligible(g.d, bd, cd, kd, ty, ngroups);
		if (!plan.g.ok) { // uniform
			skipped++;
			continue;
		}
		const RwQuarter qr(g, wave);
		if (qr.empty()) continue; // uniform per wave
		const uint4 *aseg16 = reinterpret_cast<const uint4 *>(awords + g.d.word_off);
		const uint4 *bseg16 = reinterpret_cast<const uint4 *>(bwords + bd.word_off);
		const uint4 *cseg16 = reinterpret_cast<const uint4 *>(cwords + cd.word_off);
		const RwKeyStream ks(kwords, kd);
		group_rw_dispatch(g.d.width, ks.direct(g.d.width), [&](auto wt, auto direct) __attribute__((always_inline)) {
			group_product3_walk<decltype(wt)::value, decltype(direct)::value, V, C>(
			    qr.r0, qr.r1, g.d, bd, cd, plan, aseg16, bseg16, cseg16, ks, ngroups, keys[wave],
			    bstage[wave], cstage[wave], sums + wave * kSlots, cnts + (C ? wave * kSlots : 0u), validity);
		});
	}
	if (skipped && tid == 0u) atomicAdd(fallback, (unsigned long long)skipped);
	// one partial {sum, count} per bin and workgroup
	group_rw_pairs_out<C>(sums, cnts, red, nbins, partial + (uint64_t)blockIdx.x * 2u * nbins);
}
