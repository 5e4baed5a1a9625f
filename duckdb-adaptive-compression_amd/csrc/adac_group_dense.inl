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
// types and the domain alone (dense_plan; forms.dense_form_groups is its host mirror).  This file holds the plan, the
// accumulator and the kernel; the readers themselves are adac_dense_read.inl's (included below, after the plan), shared
// with the mapped scans, and reach the accumulator through a sink (DenseSink).
//   header   the key segment has a frame (product_frame) and [frame, frame + 2^w - 1] does not meet the domain: no row
//            can contribute.  No packed word of either column and no mask word is read, nothing is added.
//   walk     key: frame, 4 <= w <= 32, count * w < 2^31 (member_plan's walk); with SUM the value column also needs a
//            frame, 1 <= w <= 32 and count * w < 2^31.  dense_key_walk.
//   staged   everything else (key widths 1..3 and 33..64, value widths above 32, raw signed slots, ADAC_NO_MIN,
//            unpacked segments, frames that wrap, the all-ones stored min): dense_key_staged_pair with SUM,
//            dense_key_staged_keys without.
//   window   the key segment has a frame and the indices its interval can reach, [lo, hi), are at most kDenseWindow:
//            the workgroup keeps a zeroed LDS window of 64-bit sums and 32-bit counts, rows add into it with LDS
//            atomics, and after the last barrier its non-zero entries go out with one global atomicAdd each.
//   direct   otherwise: global atomicAdd on d_sums + t (and d_counts + t), only when t < key_span: no out-of-range
//            address is ever formed.
//
// RUN COMBINING (walk reader, either accumulator; tuning knob group_dense_combine): a lane visits its chunk's rows in row
// order and keeps (t_cur, sum, count) in registers.  A wanted in-domain row with t == t_cur adds into the registers,
// any other wanted in-domain row flushes the pair with one atomic per output array and starts a new run, the end of the
// chunk (the sink's end()) flushes.  Masked-out rows and rows outside the domain neither flush nor join a run.  On sorted
// keys (l_orderkey: about four rows per key) that is one atomic per run and chunk where adac_scan_build_member pays one
// per row.  The staged readers end the run after every row: one atomic per row and output array there.  Integer sums
// mod 2^64 commute, so the results depend neither on the knob nor on the order the atomics arrive in.
//
// Barriers: one after the window is zeroed, one before it is written out; the staged readers have their stages' own.
// EVERY thread reaches every barrier in every form: the reader is chosen uniformly per workgroup, a wave whose quarter
// is empty, and the header form, skip only the walk.

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

#include "adac_dense_read.inl" // the readers the plan chooses among: dense_key_read, dense_key_seg_rows

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

// The readers' sink: a lane's run in front of the accumulator.  Between two end() calls the run is empty.
template <bool SUM>
struct DenseSink {
	const DenseAcc<SUM> &acc;
	bool combine; // uniform
	DenseRun<SUM> run;
	__device__ __forceinline__ void row(uint64_t t, uint64_t v) { run.row(acc, t, v, combine); }
	__device__ __forceinline__ void end() { run.flush(acc); }
};

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
	DenseSink<SUM> sink {acc, combine, {}};
	const uint32_t rows = dense_key_read<V, SUM>(g, vd, plan, kwords, vwords, dom, v_tmask, v_sbit, validity, lds, sink);
	dense_key_seg_rows(seg_rows, g.seg, rows);
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
