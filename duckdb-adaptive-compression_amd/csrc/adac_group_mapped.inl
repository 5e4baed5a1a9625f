// adac_group_mapped.inl — SUM(value), COUNT(*) GROUP BY A CODE LOOKED UP THROUGH A DENSE KEY over two packed columns of
// one table (TPC-H Q5's revenue per nation of the supplier behind l_suppkey, Q10 / Q3 through o_custkey / l_orderkey,
// Q14 / Q19 through l_partkey), and the scan that builds such a map from a dimension table with sparse keys.  Nothing is
// decoded to memory, there is no hash table and no global atomic per row.  Included into adac_kernels.hip inside
// namespace adac::{anonymous}, after adac_group_dense.inl: the kernels have k_group_dense's shell (one workgroup per
// ScanGroup of the KEY layout, the host clears the outputs, one atomicAdd per wave for the rows per segment, not
// persistent), its domain (MemberDomain), its plan (dense_plan: header / walk / staged, the value column's eligibility
// for the walk included) and its readers: adac_dense_read.inl's walk and two staged readers, which hand every wanted
// row inside the domain to a SINK.  This file holds the map's slice, the two sinks (MappedBins for the probe,
// MappedStore for the build; neither keeps a row back, so their end() is empty) and the kernels.
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

// the copies of `ngroups` bins that a kernel with `bins` LDS bins (kMappedBins, kMappedProductBins) allows: a power of
// two (host; the knob group_mapped_copies caps it)
inline uint32_t mapped_copies(uint32_t ngroups, uint32_t bins, int knob) {
	uint32_t c = 1;
	while (c * 2u * ngroups <= bins && c * 2u <= kMappedMaxCopies) c *= 2u;
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
	__device__ __forceinline__ void end() {}
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
	__device__ __forceinline__ void end() {}
};

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
	const uint32_t rows = dense_key_read<V, SUM>(g, vd, plan.p, kwords, vwords, dom, v_tmask, v_sbit, validity, lds, sink);
	dense_key_seg_rows(seg_rows, g.seg, rows);
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
	const uint32_t rows = dense_key_read<V, true>(g, cd, plan, kwords, cwords, dom, c_tmask, c_sbit, validity, lds, sink);
	dense_key_seg_rows(seg_rows, g.seg, rows);
}
