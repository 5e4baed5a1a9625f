"""One segment at and past 2^31 / 2^32 bits.

The C ABI does not assume DuckDB's 256 KiB blocks, and every kernel with a width-templated register walk hands over to
its staged (LDS) form at exactly count * w == 2^31 bits; everything else about long segments mixes 64-bit bit positions
with 32-bit row, chunk and dword arithmetic.  The hand-overs, and the file that runs each on such a segment:

  here                              k_scan_agg (SUM, COUNT(range), the selection scan), k_repack_g and
                                    k_analyze_packed_g (re-encode), the register-walk plan of the grouped scan
                                    (scan_group_sum), the product plan (scan_sum_product); encode, decode, ranges, jobs,
                                    row fetches and unpack_selected round the thresholds
  test_gpu_big_segment_scans.py     scan_group_sum_valid, scan_group_sum_product, scan_group_sum_product3,
                                    scan_group_sum_q1, the compare scans (compare_plan), the member scans (member_plan),
                                    the dense-key scans (dense_plan), the mapped scans and the map build (mapped_plan),
                                    scan_group_sum_product_mapped (mapped_product_plan); big_scan_cases.py holds its
                                    cells and test_big_scan_census.py states on the CPU what they rely on

The columns here are the smallest that cross those sizes (input bytes ~ packed bytes ~ 256 MiB per 2^31 bits):

  u32 / w 31   S0 = floor((2^31 - 1) / 31) rows (count * w < 2^31), S1 = ceil(2^31 / 31) rows (count * w >= 2^31) and a
               small S2 whose word_off lies past 2^26 words = 2^32 bits of arena: both sides of every hand-over
  i32 / w 31   S1 and S2 again, all values below zero (negative frame of reference, SEG_LINEAR)
  u64 / w 63   ceil(2^32 / 63) rows: the LAST field straddles bit 2^32 (the three-dword field reader); in that segment
               every row still STARTS below 2^32, so a second segment of 2 * TILE + 3 more rows follows, in which tiles,
               ranges and fetched rows start past bit 2^32; and a small one
  u8  / w 7    ceil(2^31 / 7) rows: element and bitmap bit indices past 2^28, bitmap dword indices past 2^23

Values are a multiplicative hash of the row number (first row 0, last row 2^w - 1, plus a frame of reference); every
expectation is numpy over those values or the oracle's packing of them."""
import numpy as np
import pytest

from test_gpu_group_sum import reference_groups
from test_gpu_parity import wide_sum
from test_gpu_sum_product import expected_sums

gpu = pytest.mark.gpu

U64 = 0xFFFFFFFFFFFFFFFF
B31, B32 = 1 << 31, 1 << 32
TILE_BYTES = 16384


def rows_below(bits, w):
    """The most rows of width w whose bits stay below `bits`."""
    return (bits - 1) // w


def rows_reaching(bits, w):
    """The fewest rows of width w that hold `bits` bits."""
    return -(-bits // w)


# name -> (dtype, [(rows, width, frame of reference as a bit pattern of the type)])
COLUMNS = {
    "u32": (np.uint32, [(rows_below(B31, 31), 31, 0x12345678), (rows_reaching(B31, 31), 31, 0x23456789), (4097, 13, 70001)]),
    "i32": (np.int32, [(rows_reaching(B31, 31), 31, 1 << 31), (4097, 13, (1 << 32) - 70000)]),
    "u64": (np.uint64, [(rows_reaching(B32, 63), 63, 12345), (rows_reaching(B32, 63) + 2 * 2048 + 3, 63, 1 << 62),
                        (4097, 40, 1 << 50)]),
    "u8": (np.uint8, [(rows_reaching(B31, 7), 7, 100), (4097, 3, 200)]),
}
BIG = {"u32": (0, 1), "i32": (0,), "u64": (0, 1), "u8": (0,)}   # the segments built round a threshold


def hashed(n, bits, base, dtype, salt=0):
    """n values of `dtype`: base + the top `bits` bits of a multiplicative hash of the row number, modulo the type;
    the first row holds base + 0 and the last base + 2^bits - 1."""
    dtype = np.dtype(dtype)
    udt = np.dtype("u%d" % dtype.itemsize)
    out = np.empty(n, dtype=udt)
    wide = np.uint64 if bits > 32 else np.uint32
    mul, top = (wide(0x9E3779B97F4A7C15), 64) if bits > 32 else (wide(0x9E3779B1), 32)
    step = 1 << 22
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        x = np.arange(lo + salt, hi + salt, dtype=wide)
        x *= mul
        x >>= wide(top - bits)
        x += wide(base & (2 ** top - 1))
        out[lo:hi] = x                     # keeps the low bits: modulo the type
    out[0] = base & (2 ** (8 * dtype.itemsize) - 1)
    out[n - 1] = (base + 2 ** bits - 1) & (2 ** (8 * dtype.itemsize) - 1)
    return out.view(dtype)


def arena_words(count, w):
    return (((count * w + 64) >> 6) + 15) & ~15


class Column:
    pass


def column_from(name, dtype, spec, big):
    """The values of a column and what an encode must find, by numpy (min / max) alone."""
    c = Column()
    c.name, c.dtype = name, np.dtype(dtype)
    c.tile = TILE_BYTES // c.dtype.itemsize
    c.counts = np.array([n for n, _, _ in spec], dtype=np.uint32)
    c.widths = [w for _, w, _ in spec]
    c.offs = [int(o) for o in np.concatenate([[0], np.cumsum(c.counts.astype(np.int64))[:-1]])]
    c.n = int(c.counts.astype(np.int64).sum())
    c.vals = np.empty(c.n, dtype=c.dtype)
    for i, (n, w, base) in enumerate(spec):
        c.vals[c.offs[i]:c.offs[i] + n] = hashed(n, w, base, c.dtype, salt=i)
    c.segs = [c.vals[o:o + int(n)] for o, n in zip(c.offs, c.counts)]
    # min / max as the append rule orders them: sign-extended to 64 bits
    c.minmax = [(int(v.min()) & U64, int(v.max()) & U64) for v in c.segs]
    c.big = big
    return c


def make_column(name):
    dtype, spec = COLUMNS[name]
    return column_from(name, dtype, spec, BIG[name])


def threshold_rows(count, w):
    """Rows of a segment whose field holds bit 2^31 or bit 2^32 of the packed stream, or starts right after it."""
    rows = []
    for bits in (B31, B32):
        r = bits // w
        rows += [x for x in (r - 1, r, r + 1) if 0 <= x < count]
    return rows


@pytest.mark.parametrize("name", list(COLUMNS))
def test_generators_land_on_both_sides_of_the_thresholds(oracle, name):
    """Held on the CPU: row counts from the formulas, widths by the reference's own rule from numpy's min / max."""
    assert rows_below(B31, 31) == 69_273_666 and rows_reaching(B31, 31) == 69_273_667
    assert rows_reaching(B32, 63) == 68_174_085 and rows_reaching(B31, 7) == 306_783_379
    c = make_column(name)
    tb = 8 * c.dtype.itemsize
    for (mn, mx), w, v in zip(c.minmax, c.widths, c.segs):
        assert oracle.width_from_succinct(mn, mx) == w and w < tb            # packs, at the width meant
        assert (int(v[0]) & U64, int(v[-1]) & U64) == (mn, mx)                # both ends of the range are present
    bits = [int(n) * w for n, w in zip(c.counts, c.widths)]
    woff = np.concatenate([[0], np.cumsum([arena_words(int(n), w) for n, w in zip(c.counts, c.widths)])])
    if name == "u32":
        assert bits[0] < B31 <= bits[1] and bits[0] + 31 >= B31 > bits[1] - 31   # the nearest counts on either side
        assert woff[2] > 1 << 26                                             # S2 starts past 2^32 bits of arena
    elif name == "i32":
        assert bits[0] >= B31 > bits[0] - 31
        assert all(int(v.max()) < 0 for v in c.segs)                         # linear: one side of zero
    elif name == "u64":
        assert bits[0] >= B32 > bits[0] - 63
        assert (int(c.counts[0]) - 1) * 63 < B32                             # ... but no row of it starts past 2^32
        assert (int(c.counts[1]) - c.tile - 3) * 63 > B32                    # the last TILE + 3 rows of the next do
    else:
        assert bits[0] >= B31 > bits[0] - 7
        assert int(c.counts[0]) > 1 << 28 and int(c.counts[0]) // 32 > 1 << 23
    for s in c.big:
        assert threshold_rows(int(c.counts[s]), c.widths[s])


# ---------------------------------------------------------------------------------------------------------------------
# the encoded column, shared by the GPU tests of one column
# ---------------------------------------------------------------------------------------------------------------------
def memset(adac, ctx, buf, byte):
    assert adac.lib().adac_dev_memset(ctx._h, buf.ptr, byte, buf.nbytes) == 0


def encoded(adac, gpu_ctx, c):
    """The column on the device: uploaded, encoded, its descriptors read back; freed after the module's last test."""
    assert adac.tile_values(c.dtype) == c.tile
    c.lay = adac.Layout(gpu_ctx, c.dtype, c.counts)
    assert c.lay.value_span == c.n
    c.d_vals = gpu_ctx.upload(c.vals)
    c.d_words = gpu_ctx.alloc(c.lay.max_arena_words * 8 + 16).zero()
    c.lay.encode(c.d_vals, c.d_words)
    gpu_ctx.sync()
    c.descs = c.lay.get_descs()
    yield c
    c.lay.close()
    c.d_vals.free()
    c.d_words.free()


@pytest.fixture(scope="module", params=list(COLUMNS))
def column(request, adac, gpu_ctx):
    yield from encoded(adac, gpu_ctx, make_column(request.param))


def check_descs(adac, c, descs, mm, widths=None, packed=None):
    widths = widths or c.widths
    woff = 0
    for s, (mn, mx) in enumerate(c.minmax):
        d = descs[s]
        assert (int(mm[s, 0]), int(mm[s, 1])) == (mn, mx), "min/max of segment %d" % s
        assert int(d["count"]) == int(c.counts[s]) and int(d["val_off"]) == c.offs[s]
        assert int(d["width"]) == widths[s], "width of segment %d" % s
        is_packed = packed[s] if packed else True
        assert bool(d["flags"] & adac.SEG_PACKED) == is_packed
        if is_packed:
            assert int(d["min"]) == adac.stored_min(mn, mx, widths[s]) == mn
        assert int(d["word_off"]) == woff
        woff += arena_words(int(c.counts[s]), widths[s])


def windows(count, w, nrows=4096):
    """(first row, rows): the head, the tail and one round each threshold bit; every window starts at a multiple of 64
    rows (so on a word) and ends on one or on the segment's last row."""
    out = [(0, min(nrows, count)), (max(0, (count - nrows) & ~63), count - max(0, (count - nrows) & ~63))]
    for bits in (B31, B32):
        r = bits // w
        if r < count:
            r0 = max(0, r - nrows // 2) & ~63
            out.append((r0, min(nrows, count - r0)))
    return out


def check_words_in_windows(oracle, c, d_words, descs, widths=None, mins=None):
    for s, v in enumerate(c.segs):
        w = (widths or c.widths)[s]
        mn = mins[s] if mins else c.minmax[s][0]
        for r0, rows in windows(len(v), w):
            exp = oracle.pack_flat(v[r0:r0 + rows], mn, w)
            got = d_words.download(np.uint64, len(exp), (int(descs[s]["word_off"]) + r0 * w // 64) * 8)
            assert np.array_equal(got, exp), "packed words of segment %d, rows %d..%d" % (s, r0, r0 + rows)


@gpu
def test_encode_both_paths(adac, oracle, gpu_ctx, column):
    c = column
    check_descs(adac, c, c.descs, c.lay.get_minmax())
    check_words_in_windows(oracle, c, c.d_words, c.descs)
    # every packed word of the big segments (the oracle packs ~10^8 rows in well under a second)
    for s in c.big:
        exp = oracle.pack_flat(c.segs[s], c.minmax[s][0], c.widths[s])
        got = c.d_words.download(np.uint64, len(exp), int(c.descs[s]["word_off"]) * 8)
        assert np.array_equal(got, exp), "packed words of segment %d" % s
        del exp, got
    # the other encode form (layouts with segments this large always take the three kernels; asked for explicitly)
    lay = adac.Layout(gpu_ctx, c.dtype, c.counts)
    d_words = gpu_ctx.alloc(lay.max_arena_words * 8 + 16).zero()
    for knob in (0, 1):
        adac.set_tuning("single_pass_encode", knob)
        try:
            memset(adac, gpu_ctx, d_words, 0)
            lay.encode(c.d_vals, d_words)
            gpu_ctx.sync()
        finally:
            adac.set_tuning("single_pass_encode", 1)
        descs = lay.get_descs()
        assert descs.tobytes() == c.descs.tobytes()
        check_descs(adac, c, descs, lay.get_minmax())
        check_words_in_windows(oracle, c, d_words, descs)
    d_words.free()


@gpu
def test_full_unpack(adac, gpu_ctx, column):
    c = column
    d_out = gpu_ctx.alloc(c.n * c.dtype.itemsize + 16)
    memset(adac, gpu_ctx, d_out, 0x5A)
    c.lay.unpack(c.d_words, d_out)
    gpu_ctx.sync()
    got = d_out.download(c.dtype, c.n)
    d_out.free()
    assert np.array_equal(got, c.vals)


def straddling_ranges(c):
    """(segment, start, count): round the threshold rows, the last TILE + 3 rows, row 0."""
    out = []
    for s in c.big:
        n, w = int(c.counts[s]), c.widths[s]
        for bits in (B31, B32):
            r = bits // w
            if r < n:
                st = max(0, r - c.tile - 5)
                out.append((s, st, min(n - st, 2 * c.tile + 11)))     # straddles the row that holds the bit
                out.append((s, r, min(n - r, c.tile)))                # starts on it
                if r + 1 < n:
                    out.append((s, r + 1, min(n - r - 1, c.tile)))    # starts past it
        out += [(s, n - c.tile - 3, c.tile + 3), (s, 0, 1), (s, 0, c.tile)]
    last = len(c.counts) - 1
    out += [(last, 0, int(c.counts[last])), (last, 1, 77)]
    return out


@gpu
def test_ranges_and_jobs_round_the_thresholds(adac, gpu_ctx, column):
    c = column
    size = c.dtype.itemsize
    ranges = straddling_ranges(c)
    poison = np.full(size, 0x77, dtype=np.uint8).view(c.dtype)[0]
    for out_off in (0, 1):
        # adac_unpack_range: one call per range, each into a poisoned buffer of its own
        for s, st, cnt in ranges:
            d_out = gpu_ctx.alloc((cnt + out_off + 16) * size)
            memset(adac, gpu_ctx, d_out, 0x77)
            c.lay.unpack_range(c.d_words, s, st, cnt, d_out, out_off)
            got = d_out.download(c.dtype, cnt + out_off + 16)
            d_out.free()
            assert np.array_equal(got[out_off:out_off + cnt], c.segs[s][st:st + cnt]), (c.name, s, st, cnt, out_off)
            assert np.all(got[:out_off] == poison) and np.all(got[out_off + cnt:] == poison)
        # adac_unpack_jobs: all of them in one call, ragged placement, output pointer off by out_off elements
        offs, run = [], 3
        for i, (_, _, cnt) in enumerate(ranges):
            offs.append(run)
            run += cnt + i % 5
        total = run + 8
        jobs = adac.jobs_from_descs([c.descs[s] for s, _, _ in ranges], [(st, cnt) for _, st, cnt in ranges], offs)
        d_dst = gpu_ctx.alloc((total + 1) * size + 64)
        memset(adac, gpu_ctx, d_dst, 0x77)
        adac.unpack_jobs(gpu_ctx, c.dtype, jobs, c.d_words, d_dst.ptr + out_off * size)
        gpu_ctx.sync()
        got = d_dst.download(c.dtype, total + 1)
        d_dst.free()
        exp = np.full(total + 1, poison, dtype=c.dtype)
        for (s, st, cnt), o in zip(ranges, offs):
            exp[out_off + o:out_off + o + cnt] = c.segs[s][st:st + cnt]
        assert np.array_equal(got, exp), (c.name, out_off)


@gpu
def test_fetch_rows_round_the_thresholds(adac, gpu_ctx, column):
    c = column
    segs, rows = [], []
    for s, n in enumerate(c.counts):
        mine = [0, int(n) - 1] + (threshold_rows(int(n), c.widths[s]) if s in c.big else [1, int(n) // 2])
        segs += [s] * len(mine)
        rows += mine
    segs, rows = np.array(segs, dtype=np.uint32), np.array(rows, dtype=np.uint32)
    d_out = gpu_ctx.alloc(len(rows) * c.dtype.itemsize + 16)
    memset(adac, gpu_ctx, d_out, 0x77)
    d_s, d_r = gpu_ctx.upload(segs), gpu_ctx.upload(rows)
    c.lay.fetch_rows(c.d_words, d_s, d_r, len(rows), d_out)
    got = d_out.download(c.dtype, len(rows))
    exp = np.array([c.segs[s][r] for s, r in zip(segs, rows)], dtype=c.dtype)
    assert np.array_equal(got, exp), (c.name, segs.tolist(), rows.tolist(), got.tolist())
    for b in (d_out, d_s, d_r):
        b.free()


def mask_words(n, salt):
    """A validity / selection mask over n elements without n random draws: hashed 64-bit words (about half the bits
    set) -> (u64 words + a spare one, bool per element)."""
    nw = (n + 63) // 64
    x = np.arange(1 + salt, nw + 1 + salt, dtype=np.uint64)
    x *= np.uint64(0xD6E8FEB86659FD93)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0x9E3779B97F4A7C15)
    words = np.concatenate([x, np.zeros(1, dtype=np.uint64)])
    keep = np.unpackbits(x.view(np.uint8), bitorder="little")[:n].view(bool)
    return words, keep


def bit_pattern(v, dtype):
    return int(np.array([v]).astype(dtype).view(np.dtype("u%d" % np.dtype(dtype).itemsize))[0])


@gpu
def test_fused_scans_on_both_sides_of_the_hand_over(adac, gpu_ctx, column):
    """SUM, COUNT(range) and the selection scan, with and without a validity mask, with the register walk allowed
    (templated_scan 1: the segments below 2^31 bits take it, the ones at or past it must not) and without."""
    c = column
    nseg = len(c.counts)
    # a band in the middle of the big segments' range, in the type's own order
    v0 = c.segs[c.big[-1]]
    a, b = int(v0[0]), int(v0[-1])
    lo, hi = a + (b - a) // 4, a + (b - a) // 2
    words, keep = mask_words(c.n, 5)
    d_valid = gpu_ctx.upload(words)
    hit = (c.vals >= c.dtype.type(lo)) & (c.vals <= c.dtype.type(hi))
    assert 0.2 < hit[:1 << 20].mean() < 0.3
    nw = (c.n + 63) // 64
    d_res = gpu_ctx.alloc(nseg * 8 + 8)
    d_bm = gpu_ctx.alloc(nw * 8 + 8)
    try:
        for valid, d_v in ((None, None), (keep, d_valid)):
            sel = hit if valid is None else hit & valid
            exp_sum = [wide_sum(v if valid is None else v[valid[o:o + len(v)]]) for v, o in zip(c.segs, c.offs)]
            exp_cnt = [int(np.count_nonzero(sel[o:o + len(v)])) for v, o in zip(c.segs, c.offs)]
            exp_bm = np.packbits(sel, bitorder="little")
            for templated in (1, 0):
                adac.set_tuning("templated_scan", templated)
                memset(adac, gpu_ctx, d_res, 0xEE)
                c.lay.scan_sum(c.d_words, d_res, d_v)
                got = d_res.download(np.uint64, nseg + 1)
                assert got[:nseg].tolist() == exp_sum, (c.name, "sum", templated, valid is not None)
                assert int(got[nseg]) == 0xEEEEEEEEEEEEEEEE
                memset(adac, gpu_ctx, d_res, 0xEE)
                c.lay.scan_count_between(c.d_words, bit_pattern(lo, c.dtype), bit_pattern(hi, c.dtype), d_res, d_v)
                got = d_res.download(np.uint64, nseg + 1)
                assert got[:nseg].tolist() == exp_cnt, (c.name, "count", templated, valid is not None)
                memset(adac, gpu_ctx, d_res, 0xEE)
                memset(adac, gpu_ctx, d_bm, 0xEE)
                c.lay.scan_select_between(c.d_words, bit_pattern(lo, c.dtype), bit_pattern(hi, c.dtype), d_bm, d_res, d_v)
                got = d_res.download(np.uint64, nseg + 1)
                assert got[:nseg].tolist() == exp_cnt, (c.name, "select", templated, valid is not None)
                bm = d_bm.download(np.uint64, nw + 1)
                assert int(bm[nw]) == 0xEEEEEEEEEEEEEEEE               # nothing past ceil(span / 64) words
                got_bm = bm[:nw].view(np.uint8)
                same = np.array_equal(got_bm[:len(exp_bm)], exp_bm) and not got_bm[len(exp_bm):].any()
                if not same:
                    bad = np.flatnonzero(got_bm[:len(exp_bm)] != exp_bm)
                    raise AssertionError((c.name, "bitmap", templated, valid is not None, bad[:4].tolist(), len(bad)))
            del exp_bm, sel
    finally:
        adac.set_tuning("templated_scan", 1)
    for b_ in (d_valid, d_res, d_bm):
        b_.free()


@gpu
def test_unpack_selected_round_the_thresholds(adac, gpu_ctx, column):
    c = column
    ids = []
    for s, n in enumerate(c.counts):
        n, o = int(n), c.offs[s]
        ids += [o, o + n - 1]
        if s in c.big:
            for r in threshold_rows(n, c.widths[s]):
                ids += [o + x for x in range(r - 40, r + 41, 3) if 0 <= x < n]
                ids += [o + x for x in (r - c.tile, r + c.tile) if 0 <= x < n]
    ids = np.unique(np.array(ids, dtype=np.int64))
    nw = (c.n + 63) // 64
    bm = np.zeros(nw + 1, dtype=np.uint64)
    np.bitwise_or.at(bm, ids >> 6, np.uint64(1) << (ids & 63).astype(np.uint64))
    d_bm = gpu_ctx.upload(bm)
    d_out = gpu_ctx.alloc((len(ids) + 16) * c.dtype.itemsize)
    d_ids = gpu_ctx.alloc((len(ids) + 16) * 8)
    memset(adac, gpu_ctx, d_out, 0x77)
    memset(adac, gpu_ctx, d_ids, 0x77)
    assert c.lay.unpack_selected(c.d_words, d_bm, d_out, d_ids) == len(ids)
    assert np.array_equal(d_ids.download(np.uint64, len(ids)), ids.astype(np.uint64))
    assert np.array_equal(d_out.download(c.dtype, len(ids)), c.vals[ids])
    for b in (d_bm, d_out, d_ids):
        b.free()


# ---------------------------------------------------------------------------------------------------------------------
# the u32 column alone: the re-encode, the grouped scan and the product scan
# ---------------------------------------------------------------------------------------------------------------------
only_u32 = pytest.mark.parametrize("column", ["u32"], indirect=True)


@gpu
@only_u32
def test_reencode_across_the_hand_over(adac, oracle, gpu_ctx, column):
    """Tight (w 31: S0 on the register walk of k_repack_g / k_analyze_packed_g, S1 on their LDS form) -> padded to
    bytes (w 32 == the type: unpacked slots, both past 2^31 bits) -> tight again; against direct encodes."""
    c = column
    padded_w = [32, 32, 16]
    packed = [False, False, True]
    direct = adac.Layout(gpu_ctx, c.dtype, c.counts)
    d_direct = gpu_ctx.alloc(direct.max_arena_words * 8 + 16).zero()
    direct.encode(c.d_vals, d_direct, pad_to_byte=True)
    gpu_ctx.sync()
    dd = direct.get_descs()
    check_descs(adac, c, dd, direct.get_minmax(), padded_w, packed)
    mins = [U64, U64, c.minmax[2][0]]                                # what the oracle subtracts: nothing from raw slots
    check_words_in_windows(oracle, c, d_direct, dd, padded_w, mins)
    pad = adac.Layout(gpu_ctx, c.dtype, c.counts)
    tight = adac.Layout(gpu_ctx, c.dtype, c.counts)
    probe = adac.Layout(gpu_ctx, c.dtype, c.counts)
    d_pad = gpu_ctx.alloc(pad.max_arena_words * 8 + 16)
    d_tight = gpu_ctx.alloc(tight.max_arena_words * 8 + 16)
    try:
        for templated in (1, 0):
            adac.set_tuning("templated_scan", templated)
            # adac_analyze_packed on its own: the min / max it leaves in the layout it filled
            for src, d_src in ((c.lay, c.d_words), (direct, d_direct)):
                src.analyze_packed(d_src, probe)
                gpu_ctx.sync()
                mm = probe.get_minmax()
                assert [(int(x), int(y)) for x, y in mm] == c.minmax, templated
            memset(adac, gpu_ctx, d_pad, 0)
            c.lay.reencode(c.d_words, pad, d_pad, pad_to_byte=True)
            gpu_ctx.sync()
            pdescs = pad.get_descs()
            assert pdescs.tobytes() == dd.tobytes(), templated
            check_words_in_windows(oracle, c, d_pad, pdescs, padded_w, mins)
            memset(adac, gpu_ctx, d_tight, 0)
            pad.reencode(d_pad, tight, d_tight)
            gpu_ctx.sync()
            tdescs = tight.get_descs()
            assert tdescs.tobytes() == c.descs.tobytes(), templated
            check_descs(adac, c, tdescs, tight.get_minmax())
            check_words_in_windows(oracle, c, d_tight, tdescs)
    finally:
        adac.set_tuning("templated_scan", 1)
    for b in (d_direct, d_pad, d_tight):
        b.free()


def small_keys(n, ngroups):
    """n uint8 group keys below `ngroups`: a second hash of the row number."""
    keys = np.empty(n, dtype=np.uint8)
    for lo in range(0, n, 1 << 22):
        hi = min(n, lo + (1 << 22))
        x = np.arange(lo, hi, dtype=np.uint32)
        x *= np.uint32(0x85EBCA6B)
        keys[lo:hi] = (x >> np.uint32(16)) % np.uint32(ngroups)
    return keys


@gpu
@only_u32
def test_group_sum_across_the_hand_over(adac, gpu_ctx, column):
    c = column
    keys = small_keys(c.n, 6)
    klay = adac.Layout(gpu_ctx, np.uint8, c.counts)
    d_keys = gpu_ctx.upload(keys)
    d_kwords = gpu_ctx.alloc(klay.max_arena_words * 8 + 16).zero()
    klay.encode(d_keys, d_kwords)
    gpu_ctx.sync()
    assert klay.get_descs()["width"].tolist() == [3, 3, 3]
    exp_s, exp_c = reference_groups(c.vals, keys, 6)
    assert exp_c[6] == 0 and min(exp_c[:6]) > 0
    d_sums = gpu_ctx.alloc(7 * 8)
    d_cnts = gpu_ctx.alloc(7 * 8)
    try:
        for rw in (1, 0, 1):
            adac.set_tuning("group_sum_rw", rw)
            memset(adac, gpu_ctx, d_sums, 0xEE)
            memset(adac, gpu_ctx, d_cnts, 0xEE)
            c.lay.scan_group_sum(c.d_words, klay, d_kwords, 6, d_sums, d_cnts)
            assert d_cnts.download(np.uint64, 7).tolist() == exp_c, rw
            assert d_sums.download(np.uint64, 7).tolist() == exp_s, rw
    finally:
        adac.set_tuning("group_sum_rw", 1)
    for b in (d_keys, d_kwords, d_sums, d_cnts):
        b.free()


@gpu
@only_u32
def test_sum_product_across_the_hand_over(adac, gpu_ctx, column):
    """The big column on side a, a narrow u16 column on side b, then the sides swapped (the guard looks at either)."""
    c = column
    nseg = len(c.counts)
    other = hashed(c.n, 5, 1000, np.uint16, salt=7)
    olay = adac.Layout(gpu_ctx, np.uint16, c.counts)
    d_other = gpu_ctx.upload(other)
    d_owords = gpu_ctx.alloc(olay.max_arena_words * 8 + 16).zero()
    olay.encode(d_other, d_owords)
    gpu_ctx.sync()
    assert all(w <= 5 for w in olay.get_descs()["width"].tolist())
    words, keep = mask_words(c.n, 11)
    d_valid = gpu_ctx.upload(words)
    d_sums = gpu_ctx.alloc(nseg * 8 + 8)
    for valid, d_v in ((None, None), (keep, d_valid)):
        exp = expected_sums(c.vals, other, c.counts, valid)
        for a, aw, b, bw in ((c.lay, c.d_words, olay, d_owords), (olay, d_owords, c.lay, c.d_words)):
            memset(adac, gpu_ctx, d_sums, 0xFF)
            a.scan_sum_product(aw, b, bw, d_sums, d_v)
            got = d_sums.download(np.uint64, nseg + 1)
            assert [int(x) for x in got[:nseg]] == exp, (a is c.lay, valid is not None)
            assert int(got[nseg]) == U64
    for b_ in (d_other, d_owords, d_valid, d_sums):
        b_.free()
