// adac_chunk_walk.inl — the parts every width-templated register walk shares (field_of's callers: scan_run_w,
// repack_run_w, analyze_run_w, group_rw_walk, product_walk).  Included into adac_kernels.hip inside
// namespace adac::{anonymous}, after field_of.
//
// The walk: rows [r0, r1) of a segment packed at W bits (4 <= W <= 32; 2 and 3 in the narrow scan), r0 a multiple of
// 128 rows so that its bits start a 16-byte chunk, the segment below 2^31 bits.  A walker (a lane) owns whole chunks
// L = c0 + its index, + its stride, ... < c1 and decodes the rows that START in its chunk.  Per chunk it loads the chunk
// and the dword after it — a round ahead, unconditionally, the index clamped into the segment — and shifts the 160-bit
// window once so that the first row starting in the chunk sits at bit 0 (ChunkWindow); field_of then finds every row
// at a compile-time position.  Who walks (a workgroup, a wave, some lanes of a wave) and with which stride stays
// with the caller, and so does everything that is done with the fields.

// The chunks that hold the rows [r0, r1) of a segment of `count` rows
template <int W>
struct ChunkRange {
	uint32_t c0, c1; // chunks [c0, c1) hold a bit of the run
	uint32_t clast;  // last chunk holding data bits of the segment
	__device__ __forceinline__ ChunkRange(uint32_t r0, uint32_t r1, uint32_t count)
	    : c0((uint32_t)(((uint64_t)r0 * W) >> 7)), c1((uint32_t)(((uint64_t)r1 * W + 127) >> 7)),
	      clast((uint32_t)(((uint64_t)count * W + 127) >> 7) - 1) {}
	// what load() reads for chunk L (a walker past the run, or the prefetch past its last chunk: any data will do)
	__device__ __forceinline__ uint32_t clamp(uint32_t L) const { return L < clast ? L : clast; }
	// chunk L and the dword after it.  The dword after the LAST chunk is never part of a row: the chunk's own first
	// dword is read in its place.
	__device__ __forceinline__ void load(const uint4 *__restrict__ seg16, uint32_t L, uint4 &q, uint32_t &e) const {
		const uint32_t Lc = clamp(L);
		q = seg16[Lc];
		e = reinterpret_cast<const uint32_t *>(seg16 + (Lc < clast ? Lc + 1 : clast))[0];
	}
};

// first row starting in chunk L
template <int W>
__device__ __forceinline__ uint32_t chunk_first_row(uint32_t L) {
	return (128u * L + (W - 1)) / W;
}

// Chunk L (q, the dword after it e) of a run that ends at row r1, normalised
template <int W>
struct ChunkWindow {
	static constexpr int MAXV = (128 + W - 1) / W; // rows starting in a chunk: MAXV - 1 or MAXV
	uint32_t nrm[5];                               // the window from row i0's first bit on: field_of<W>(nrm, j) = row i0 + j
	uint32_t i0;                                   // first row starting in the chunk
	uint32_t o0;                                   // its bit offset in the chunk, < W <= 32
	uint32_t starting;                             // rows starting in the chunk
	uint32_t lim;                                  // rows from i0 to the end of the run (0 for a walker past it)
	__device__ __forceinline__ ChunkWindow(const uint4 &q, uint32_t e, uint32_t L, uint32_t r1) {
		i0 = chunk_first_row<W>(L);
		o0 = i0 * W - 128u * L;
		nrm[0] = __builtin_amdgcn_alignbit(q.y, q.x, o0);
		nrm[1] = __builtin_amdgcn_alignbit(q.z, q.y, o0);
		nrm[2] = __builtin_amdgcn_alignbit(q.w, q.z, o0);
		nrm[3] = __builtin_amdgcn_alignbit(e, q.w, o0);
		nrm[4] = e >> o0;
		starting = (128u - o0 + (W - 1)) / W;
		lim = r1 > i0 ? r1 - i0 : 0u;
	}
	// rows of the run that start in the chunk; starting <= lim: an interior chunk, every row that starts in it counts
	__device__ __forceinline__ uint32_t have() const { return starting < lim ? starting : lim; }
	// for walks that unroll MAXV - 1 rows without a test: does row MAXV - 1 start in the chunk too?
	__device__ __forceinline__ bool last_starts() const { return 128 % W == 0 || starting == (uint32_t)MAXV; }
};

// The validity (or selection) mask of a run, for the walks that take one (V; without it nothing here is evaluated):
// the two 64-bit words that hold the bits of a chunk's rows travel with the chunk — requested a round ahead,
// unconditionally, word indices (relative to the segment's first word) clamped to the word of the run's last row.
// Looked up inside the loop after the walk, the mask cost the masked scans 15 - 40 % (u64 w 8: SUM 5.07 -> 3.16 TB/s).
// Not validity_window / validity_window_pair: those serve the per-row kernels.
template <int W, bool V>
struct ChunkMask {
	const uint64_t *__restrict__ vseg; // the word of the segment's element 0
	uint32_t vsh0;                     // that element's bit in it
	uint32_t vend;                     // word of the run's last row
	uint32_t r1;
	__device__ __forceinline__ ChunkMask(const uint64_t *__restrict__ validity, uint64_t val_off, uint32_t r1_)
	    : vseg(V ? validity + (val_off >> 6) : nullptr), vsh0((uint32_t)(val_off & 63u)), vend((vsh0 + r1_ - 1u) >> 6),
	      r1(r1_) {}
	// the words for chunk Lx (a chunk load() reads: clamped)
	__device__ __forceinline__ void words(uint32_t Lx, uint64_t &m0, uint64_t &m1) const {
		const uint32_t ix0 = chunk_first_row<W>(Lx);
		const uint32_t wi = (vsh0 + (ix0 < r1 ? ix0 : r1)) >> 6;
		m0 = vseg[wi < vend ? wi : vend];
		m1 = vseg[wi + 1u < vend ? wi + 1u : vend];
	}
	// the 64 mask bits from row `at` on (bits past the run's last row are unspecified)
	__device__ __forceinline__ uint64_t window(uint64_t m0, uint64_t m1, uint32_t at) const {
		const uint32_t sh = (vsh0 + at) & 63u;
		return (m0 >> sh) | ((m1 << 1) << (63u - sh));
	}
};

// f(std::integral_constant<int, w>) for the widths the register walks are instantiated at; any other w: nothing.
// The callers pass a generic lambda marked always_inline, like the walks it calls.
template <typename F>
__device__ __forceinline__ void dispatch_width_4_32(uint32_t w, F &&f) {
	switch (w) { // uniform
#define ADAC_W(N) case N: f(std::integral_constant<int, N> {}); break;
		ADAC_W(4) ADAC_W(5) ADAC_W(6) ADAC_W(7) ADAC_W(8) ADAC_W(9) ADAC_W(10) ADAC_W(11) ADAC_W(12) ADAC_W(13)
		ADAC_W(14) ADAC_W(15) ADAC_W(16) ADAC_W(17) ADAC_W(18) ADAC_W(19) ADAC_W(20) ADAC_W(21) ADAC_W(22)
		ADAC_W(23) ADAC_W(24) ADAC_W(25) ADAC_W(26) ADAC_W(27) ADAC_W(28) ADAC_W(29) ADAC_W(30) ADAC_W(31) ADAC_W(32)
#undef ADAC_W
	default: break;
	}
}
