// adac_group_rw_walk.inl — what the succinct side's register-walk ("rw") grouped scans share: k_group_sum_rw
// (adac_group_sum.inl), k_group_product_rw, k_group_product3_rw, k_group_q1_rw and, for the quartering, k_scan_product
// (adac_sum_product.inl).  Included into adac_kernels.hip inside namespace adac::{anonymous}, after adac_chunk_walk.inl
// and before the five.
//
// Every one of them gives a quarter of a scan group to ONE wave, and the four grouped ones read the keys of a round's
// rows the same way.  Written here once:
//   RwKeys<W, DIRECT>    the key reader of the four grouped walks (and its free functions group_rw_key_*);
//   RwQuarter, RwKeyStream, group_rw_dispatch, group_rw_pairs_out: the kernels' shell around the walk.
// The walk bodies stay separate functions: the round loop, the staged columns, the BATCH of field reads, the row
// arithmetic and the LDS adds.  The rule for what they share: small pieces that a walk instantiates BY NAME — never a
// walk templated over the number of columns.  The staged column is not such a piece yet: as a struct it
// cost the product kernels 9 - 19 VGPRs.

// (these four are used before adac_group_sum.inl's own kGroup* constants are seen, hence here)
constexpr uint32_t kGroupPrivateBins = 8;     // bins held per thread (staged kernels, rw kernels, host launchers)
constexpr uint32_t kGroupRwCopies = 32;       // bin sets per wave of the rw kernels (two lanes share a set)
constexpr uint32_t kGroupRwWaveRows = 1008;                    // key rows a wave stages per round: two 8-row blocks per lane
constexpr uint32_t kGroupRwWaveKeyBytes = kGroupRwWaveRows + 16 + 64; // + the block the round starts in + read slack

// A scan group in four contiguous quarters of whole 128-row units (a quarter's bits start a 16-byte chunk of `a`), one
// per wave: rows [r0, r1) of the segment.  empty(): the group has no rows for this wave (uniform per wave).
struct RwQuarter {
	uint32_t r0, r1;
	bool none;
	__device__ __forceinline__ RwQuarter(const ScanGroup &g, uint32_t wave) {
		constexpr uint32_t kWaves = kWorkgroup / 64;
		const uint32_t per = (((g.n + kWaves - 1u) / kWaves) + 127u) & ~127u;
		const uint32_t q0 = wave * per;
		none = q0 >= g.n;
		r0 = g.first + q0;
		r1 = g.first + (q0 + per < g.n ? q0 + per : g.n);
	}
	__device__ __forceinline__ bool empty() const { return none; }
};

// a segment's key stream as the grouped walks read it
struct RwKeyStream {
	const uint32_t *kw32;
	uint32_t wk;
	uint32_t k_last; // its last dword holding data bits
	__device__ __forceinline__ RwKeyStream(const uint64_t *__restrict__ kwords, const adac_segment_desc &kd)
	    : kw32(reinterpret_cast<const uint32_t *>(kwords + kd.word_off)), wk(kd.width),
	      k_last((uint32_t)(((uint64_t)kd.count * wk + 31) >> 5) - 1u) {}
	// do the keys of the rows of one chunk of an `a` of width wa fit one dword?  (uniform; the walks' DIRECT form)
	__device__ __forceinline__ bool direct(uint32_t wa) const { return ((128u + wa - 1u) / wa) * wk <= 32u; }
};

// ------------------------------------------------------------------------------------------------------------------
// Keys.  Two forms, uniform per segment pair:
//   DIRECT   the keys of a chunk's rows fit one dword (MAXV * wk <= 32: every value width >= 11 at wk = 3): a lane
//            loads the two dwords of the key stream that hold them (prefetched a round ahead like its value chunk),
//            shifts once, and finds key j with one v_bfe at the wave-uniform position j * wk.  No LDS for the keys.
//   staged   otherwise: the wave stages the key BYTES of the round's rows in a buffer of its own (8 rows per lane,
//            compile-time key width), and a lane fetches the bytes of its rows with dword reads + v_alignbyte.  LDS
//            operations of one wave are executed in order, so no barrier is needed here either.
// Key staging: the keys of an 8-row block `q` are the wk BYTES [q * wk, (q + 1) * wk) of the key stream.  A lane loads
// the three dwords that hold them (the last one may be the segment's padding word: every segment owns at least one
// 64-bit word past its data) ...
__device__ __forceinline__ void group_rw_key_load(const uint32_t *__restrict__ kw32, uint32_t q, uint32_t wk,
                                                  uint32_t last_dword, uint32_t (&d)[3], uint32_t &byte_sh) {
	const uint32_t byte0 = q * wk;
	uint32_t dw = byte0 >> 2;
	dw = dw < last_dword ? dw : last_dword; // blocks past the segment's end are never read: any data will do
	byte_sh = byte0 & 3u;
	d[0] = kw32[dw];
	d[1] = kw32[dw + 1];                     // <= last_dword + 1: inside the padding word
	d[2] = kw32[dw + 2 <= last_dword + 1u ? dw + 2 : dw + 1];
}

// ... and takes them apart at a compile-time key width: 8 keys -> 8 bytes, the frame of reference added to four at a time
template <int WK>
__device__ __forceinline__ uint2 group_rw_key_decode(const uint32_t (&d)[3], uint32_t byte_sh, uint32_t kadd4) {
	const uint32_t w0 = __builtin_amdgcn_alignbyte(d[1], d[0], byte_sh), w1 = __builtin_amdgcn_alignbyte(d[2], d[1], byte_sh);
	constexpr uint32_t mask = (1u << WK) - 1u;
	uint32_t out[2];
#pragma unroll
	for (int g = 0; g < 2; g++) {
		uint32_t acc = 0;
#pragma unroll
		for (int b = 0; b < 4; b++) {
			const int pos = (4 * g + b) * WK, dw = pos >> 5, sh = pos & 31; // pos + WK <= 64
			const uint32_t lo = dw ? w1 : w0;
			const uint32_t f = sh + WK <= 32 ? ((lo >> sh) & mask) : (__builtin_amdgcn_alignbit(w1, w0, sh) & mask);
			acc |= f << (8 * b);
		}
		out[g] = acc + kadd4; // four keys at once: no byte carries (field + kadd <= 255)
	}
	return make_uint2(out[0], out[1]);
}

__device__ __forceinline__ void group_rw_key_store(const uint32_t (&d)[3], uint32_t byte_sh, uint32_t wk, uint32_t kadd4,
                                                   bool overflow, uint2 *dst) {
	if (overflow) {
		*dst = make_uint2(~0u, ~0u);
		return;
	}
	switch (wk) { // uniform
	case 1: *dst = group_rw_key_decode<1>(d, byte_sh, kadd4); break;
	case 2: *dst = group_rw_key_decode<2>(d, byte_sh, kadd4); break;
	case 3: *dst = group_rw_key_decode<3>(d, byte_sh, kadd4); break;
	case 4: *dst = group_rw_key_decode<4>(d, byte_sh, kadd4); break;
	case 5: *dst = group_rw_key_decode<5>(d, byte_sh, kadd4); break;
	case 6: *dst = group_rw_key_decode<6>(d, byte_sh, kadd4); break;
	case 7: *dst = group_rw_key_decode<7>(d, byte_sh, kadd4); break;
	default: *dst = group_rw_key_decode<8>(d, byte_sh, kadd4); break;
	}
}

// The key reader of one wave's walk over a column of width W that ends at row r1, `lanes` chunks per round.  `keys`: the
// wave's kGroupRwWaveKeyBytes of LDS (staged form only).  Per round, in this order:
//   request(first chunk of the NEXT round, the lane's clamped chunk of the next round)   before the round is walked
//   window(cw.i0, kwin, kn), then bin(kwin, kn, j, ngroups) for the rows j of the chunk  in the walker branch
//   commit()                                                                             after the round's reads
// first() does for the first round what request() + commit() do for the others.  The window — `kwin` (DIRECT: the keys
// of rows i0 .. from bit 0) and `kn[KD]` (staged: their bytes) — is the WALK's local pair, not a member.  group_rw_walk
// writes window() out (its kernel sits at the 72 VGPRs of seven waves per SIMD and spills with the call), and
// group_product3_walk calls commit() before its columns' stores; both keep the parent's registers that way.
template <int W, bool DIRECT>
struct RwKeys {
	static constexpr int MAXV = ChunkWindow<W>::MAXV;
	static constexpr int KD = (MAXV + 3 + 3) / 4; // dwords holding MAXV bytes from any byte offset
	static constexpr uint32_t LANES = (kGroupRwWaveRows * W / 128) < 64u ? (kGroupRwWaveRows * W / 128) : 64u; // per round
	static constexpr uint32_t PASSES = ((LANES * 128u / W + 8u + 7u) / 8u + 63u) / 64u; // 8-row blocks per round / 64 lanes
	const uint32_t *__restrict__ kw32;
	const uint32_t k_last_dword, wk, kadd_byte;
	const bool keys_overflow;
	const uint32_t kadd4;
	uint8_t *const keys;
	const uint32_t r1, lanes, lane;
	uint2 kq = make_uint2(0u, 0u), kqn = make_uint2(0u, 0u); // DIRECT: this round's two dwords, the next round's
	uint32_t kb0 = 0, kb0n = 0, nblocksn = 0; // staged: first row of the buffer; the next round's, its 8-row blocks
	uint32_t kd[PASSES][3], ksh[PASSES];                      // staged: the next round's dwords of the key stream

	__device__ __forceinline__ RwKeys(const RwKeyStream &ks, uint32_t kadd_byte_, bool keys_overflow_, uint8_t *keys_,
	                                  uint32_t r1_, uint32_t lanes_)
	    : kw32(ks.kw32), k_last_dword(ks.k_last), wk(ks.wk), kadd_byte(kadd_byte_), keys_overflow(keys_overflow_),
	      kadd4(keys_overflow_ ? 0u : kadd_byte_ * 0x01010101u), keys(keys_), r1(r1_), lanes(lanes_),
	      lane(threadIdx.x & 63u) {}

	// DIRECT: the two dwords of the key stream holding the keys of the rows that start in chunk Lx
	__device__ __forceinline__ uint2 direct_keys(uint32_t Lx) const {
		uint32_t dw = (chunk_first_row<W>(Lx) * wk) >> 5;
		dw = dw < k_last_dword ? dw : k_last_dword; // (chunks past the run: any data will do)
		return make_uint2(kw32[dw], kw32[dw + 1]);   // dw + 1 <= last data dword + 1: inside the padding word
	}
	// staged: the key rows of the round that starts at chunk `rc` = [first row starting in chunk rc, first row starting
	// in chunk rc + lanes), from the 8-row block the round starts in
	__device__ __forceinline__ void round_keys(uint32_t rc, uint32_t &b0, uint32_t &nblocks) const {
		const uint32_t rows_lo = chunk_first_row<W>(rc);
		b0 = rows_lo & ~7u;
		uint32_t rows_hi = chunk_first_row<W>(rc + lanes);
		rows_hi = rows_hi < r1 ? rows_hi : r1;
		nblocks = rows_hi > b0 ? (rows_hi - b0 + 7u) >> 3 : 0u;
	}
	__device__ __forceinline__ void load_blocks(uint32_t b0) {
#pragma unroll
		for (uint32_t p = 0; p < PASSES; p++) group_rw_key_load(kw32, (b0 >> 3) + lane + 64u * p, wk, k_last_dword, kd[p], ksh[p]);
	}
	__device__ __forceinline__ void store_blocks(uint32_t nblocks) {
#pragma unroll
		for (uint32_t p = 0; p < PASSES; p++) {
			if (lane + 64u * p < nblocks) {
				group_rw_key_store(kd[p], ksh[p], wk, kadd4, keys_overflow, reinterpret_cast<uint2 *>(keys) + lane + 64u * p);
			}
		}
	}

	// the first round: it starts at chunk c0; Lc = the lane's chunk, clamped into the segment
	__device__ __forceinline__ void first(uint32_t c0, uint32_t Lc) {
		if (DIRECT) {
			kq = direct_keys(Lc);
		} else {
			uint32_t nblocks = 0;
			round_keys(c0, kb0, nblocks);
			load_blocks(kb0);
			store_blocks(nblocks);
		}
	}
	// the next round: it starts at chunk rc; Lc = the lane's chunk of it, clamped into the segment
	__device__ __forceinline__ void request(uint32_t rc, uint32_t Lc) {
		if (DIRECT) {
			kqn = direct_keys(Lc);
		} else {
			round_keys(rc, kb0n, nblocksn);
			load_blocks(kb0n);
		}
	}
	// the keys of rows [i0, i0 + MAXV), i0 = the first row starting in the lane's chunk
	__device__ __forceinline__ void window(uint32_t i0, uint32_t &kwin, uint32_t (&kn)[KD]) const {
		kwin = 0;
		if (DIRECT) {
			kwin = __builtin_amdgcn_alignbit(kq.y, kq.x, (i0 * wk) & 31u);
		} else {
			// their bytes: dword reads from the byte offset rounded down, one v_alignbyte each
			const uint32_t kofs = i0 - kb0;
			const uint32_t *k32 = reinterpret_cast<const uint32_t *>(keys) + (kofs >> 2);
			uint32_t raw[KD + 1];
#pragma unroll
			for (int i = 0; i <= KD; i++) raw[i] = k32[i];
#pragma unroll
			for (int i = 0; i < KD; i++) kn[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], kofs & 3u);
		}
	}
	// the bin of row i0 + j: its key, or `ngroups` when the key is not below it
	__device__ __forceinline__ uint32_t bin(uint32_t kwin, const uint32_t (&kn)[KD], int j, uint32_t ngroups) const {
		uint32_t key;
		if (DIRECT) {
			key = keys_overflow ? 255u : __builtin_amdgcn_ubfe(kwin, (uint32_t)j * wk, wk) + kadd_byte;
		} else {
			key = (kn[j >> 2] >> (8 * (j & 3))) & 0xffu;
		}
		return key < ngroups ? key : ngroups;
	}
	// the round's reads of the buffer are issued: the next round's key bytes take their place
	__device__ __forceinline__ void commit() {
		kq = kqn;
		if (!DIRECT) {
			store_blocks(nblocksn);
			kb0 = kb0n;
		}
	}
};


// f(std::integral_constant<int, w>, std::bool_constant<direct>) for the widths and key forms the grouped walks are
// instantiated at.  `direct` is uniform (RwKeyStream::direct).  f: a generic lambda marked always_inline.
template <typename F>
__device__ __forceinline__ void group_rw_dispatch(uint32_t w, bool direct, F &&f) {
	if (direct) {
		dispatch_width_4_32(w, [&](auto wc) __attribute__((always_inline)) { f(wc, std::true_type {}); });
	} else {
		dispatch_width_4_32(w, [&](auto wc) __attribute__((always_inline)) { f(wc, std::false_type {}); });
	}
}

// The end of a kernel whose waves hold kGroupPrivateBins x kGroupRwCopies {sum} (and, with C, {count}) words each:
// one partial {sum, count} per bin and workgroup.  kWaves x kGroupRwCopies bin words per bin, one per lane of the first
// two waves.  Holds the kernel's last two barriers: every thread of the workgroup calls it.
template <bool C>
__device__ __forceinline__ void group_rw_pairs_out(const unsigned long long *sums, const uint32_t *cnts,
                                                   unsigned long long (&red)[2][2 * kGroupPrivateBins], uint32_t nbins,
                                                   unsigned long long *__restrict__ mine) {
	constexpr uint32_t kWaves = kWorkgroup / 64;
	constexpr uint32_t kSlots = kGroupPrivateBins * kGroupRwCopies;
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
	__syncthreads();
	static_assert(kWaves * kGroupRwCopies == 128u, "two waves read a bin's words");
	if (tid < 128u) { // uniform per wave
		const uint32_t w = tid >> 5, set = tid & 31u;
		for (uint32_t b = 0; b < nbins; b++) { // uniform
			const uint64_t s = wave_sum((uint64_t)sums[w * kSlots + b * kGroupRwCopies + set]);
			const uint64_t c = C ? wave_sum((uint64_t)cnts[w * kSlots + b * kGroupRwCopies + set]) : 0ull;
			if (lane == 0u) {
				red[wave][2u * b] = s;
				red[wave][2u * b + 1u] = c;
			}
		}
	}
	__syncthreads();
	if (tid < 2u * nbins) mine[tid] = red[0][tid] + red[1][tid];
}
