"""Range decodes whose first row does not sit on a 128-bit boundary of the packed stream.

A full adac_unpack starts every tile at a multiple of the tile size, so bit0 = first * w mod 128 is always 0 there; only
adac_unpack_range and adac_unpack_jobs (the two calls an engine scans through) stage an image whose first field sits at
bit0 != 0.  Here: every type, every width 1..8*sizeof(T), every reachable bit0 on the full-tile fast paths
(decode_full_tile, decode_full_tile_u8<W>: n == TILE and output chunk alignment 0), the row-by-row path at every output
alignment and at counts round the chunk and tile sizes, ranges that end on the segment's last row, and the point fetch at
every bit phase of a 64-bit word.  Expected values are the original numpy values; for the all-NULL segment what the
oracle decodes from the words the oracle packed."""
import numpy as np
import pytest

from test_gpu_parity import make_values, oracle_encode, run_encode_decode

gpu = pytest.mark.gpu

TYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
TILE_BYTES = 16384                    # adac.tile_values(dtype) * itemsize; asserted in the fixture
EDGE_STARTS = (0, 1, 63, 64, 65, 127)
POISON = 0x77


def tile_of(dtype):
    return TILE_BYTES // np.dtype(dtype).itemsize


def chunk_of(dtype):
    """K: rows per 16-byte chunk of the output."""
    return 16 // np.dtype(dtype).itemsize


def phase_column(dtype):
    """One segment per width 1..tb of 3 * TILE + 17 rows (the one at tb cannot shrink and stays unpacked), then one
    all-NULL segment: (counts, seg_vals, validity words, index of the NULL segment).  Signed types: every packed
    segment lies below zero, so the frame of reference that the decode adds back is negative."""
    dtype = np.dtype(dtype)
    tb = 8 * dtype.itemsize
    rows = 3 * tile_of(dtype) + 17
    rng = np.random.default_rng(7100 + tb + (dtype.kind == "i"))
    segs = []
    for w in range(1, tb + 1):
        if w == tb:
            base = 0                                              # the whole range of T: mixed sign for signed T
        elif dtype.kind == "i":
            base = 2 ** (tb - 1) + (2 ** (tb - 1) - 2 ** w) // 3   # bit patterns of negative values only
        else:
            base = (2 ** tb - 2 ** w) // 3 + 1
        segs.append(make_values(rng, dtype, rows, w, base=base))
    segs.append(make_values(rng, dtype, rows, min(5, tb - 1), base=3))    # its rows are all NULL
    counts = np.full(len(segs), rows, dtype=np.uint32)
    valid = np.ones(rows * len(segs), dtype=bool)
    valid[rows * tb:] = False
    b = np.packbits(valid, bitorder="little")
    validity = np.concatenate([b, np.zeros((-len(b)) % 8 + 8, np.uint8)]).view(np.uint64)
    return counts, segs, validity, tb


def place(cursor, gap, align, k):
    """The first element offset >= cursor + gap whose chunk alignment (offset mod K) is `align`."""
    o = cursor + gap
    return o + (align - o) % k


def fast_path_jobs(counts, tile, k):
    """Every segment x every start 0..127 at count == TILE and output alignment 0: (seg, start, count, out_off)."""
    jobs, run = [], 0
    for s in range(len(counts)):
        for start in range(128):
            o = place(run, (start * 7 + s) % 3 * k, 0, k)
            jobs.append((s, start, tile, o))
            run = o + tile
    return jobs, run


def edge_counts(tile, k):
    return (1, k - 1, k, k + 1, tile - 1, tile + 1, 2 * tile + 3)


def edge_jobs(counts, tile, k):
    """Six start phases and the start that ends the range on the segment's last row x every output alignment x counts
    round the chunk and the tile."""
    jobs, run, i = [], 0, 0
    for s, n in enumerate(counts):
        for c in edge_counts(tile, k):
            for start in EDGE_STARTS + (int(n) - c,):
                for align in range(k):
                    o = place(run, i % 4, align, k)
                    jobs.append((s, start, c, o))
                    run = o + c
                    i += 1
    return jobs, run


def range_cases(counts, tile, k):
    """adac_unpack_range: the six phases and the range that ends on the last row, alignments 0 and 1, three counts."""
    jobs, run, i = [], 0, 0
    for s, n in enumerate(counts):
        for c in (1, tile, tile + 1):
            for start in EDGE_STARTS + (int(n) - c,):
                for align in (0, 1):
                    o = place(run, i % 3, align, k)
                    jobs.append((s, start, c, o))
                    run = o + c
                    i += 1
    return jobs, run


@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
def test_job_lists_reach_every_width_and_bit_phase(oracle, dtype):
    """Held on the CPU.  By the reference's own width rule segment i packs at w = i + 1 (the last width stays unpacked,
    the NULL segment has no min), and the fast-path list reaches every pair (w, bit0) a range can produce,
    bit0 in {s * w mod 128 : 0 <= s < 128}, with n == TILE and chunk alignment 0; the edge list crosses the start
    phases with every alignment and every count, inside the segments and up to their last row."""
    dtype = np.dtype(dtype)
    tile, k = tile_of(dtype), chunk_of(dtype)
    counts, segs, validity, tb = phase_column(dtype)
    enc = oracle_encode(oracle, segs, 0, False, validity, np.arange(len(segs), dtype=np.uint64) * int(counts[0]))
    assert [e[2] for e in enc[:tb]] == list(range(1, tb + 1))
    assert [e[3] for e in enc[:tb]] == [True] * (tb - 1) + [False]
    assert enc[tb][0] == 0xFFFFFFFFFFFFFFFF                      # no valid row: the min stays ADAC_NO_MIN
    widths = [e[2] for e in enc]
    if dtype.kind == "i":
        assert all((v < 0).all() for v in segs[:tb - 1])
        assert (segs[tb - 1] < 0).any() and (segs[tb - 1] > 0).any()
    fast, total = fast_path_jobs(counts, tile, k)
    reached = {(widths[s], start * widths[s] % 128) for s, start, c, o in fast if c == tile and o % k == 0}
    wanted = {(w, s * w % 128) for w in set(widths) for s in range(128)}
    assert reached == wanted
    assert any(b0 for _, b0 in reached)
    edges, _ = edge_jobs(counts, tile, k)
    per_seg = len(edge_counts(tile, k)) * (len(EDGE_STARTS) + 1) * k
    assert len(edges) == per_seg * len(counts)
    for s, n in enumerate(counts):
        mine = [(st, c, o % k) for ss, st, c, o in edges if ss == s]
        assert {a for _, _, a in mine} == set(range(k))
        assert {c for _, c, _ in mine} == set(edge_counts(tile, k))
        assert {(st, c) for st, c, _ in mine} >= {(int(n) - c, c) for c in edge_counts(tile, k)}
        assert {st for st, _, _ in mine} >= set(EDGE_STARTS)
    for lst in (fast, edges, range_cases(counts, tile, k)[0]):
        prev_end = 0
        for s, st, c, o in lst:                                   # inside the segment, ranges disjoint and ascending
            assert 0 <= st and st + c <= int(counts[s]) and c >= 1 and o >= prev_end
            prev_end = o + c


class Column:
    pass


@pytest.fixture(scope="module", params=TYPES, ids=lambda t: np.dtype(t).name)
def column(request, adac, oracle, gpu_ctx):
    dtype = np.dtype(request.param)
    assert adac.tile_values(dtype) == tile_of(dtype)
    counts, segs, validity, tb = phase_column(dtype)
    c = Column()
    c.dtype, c.tile, c.k, c.tb, c.counts = dtype, tile_of(dtype), chunk_of(dtype), tb, counts
    # encode and full decode against the oracle, word for word (bit0 == 0 everywhere in this part)
    c.lay, c.d_words, _, c.descs, _ = run_encode_decode(adac, oracle, gpu_ctx, dtype, counts, segs, validity=validity)
    assert c.descs["width"].tolist()[:tb] == list(range(1, tb + 1))
    assert all(c.descs["flags"][:tb - 1] & adac.SEG_PACKED) and not c.descs["flags"][tb - 1] & adac.SEG_PACKED
    assert int(c.descs["min"][tb]) == adac.NO_MIN
    # what a decode of each segment must give: the values, and for the NULL segment the oracle's reading (add 0) of
    # the words the oracle packed
    rows = int(counts[0])
    mn, mx, w, packed, words = oracle_encode(oracle, segs[tb:], 0, False, validity, [rows * tb])[0]
    c.expect = list(segs[:tb]) + [oracle.unpack_flat(words, 0, rows, w, 0, dtype)]
    yield c
    c.lay.close()
    c.d_words.free()


def poisoned(dtype, n):
    return np.full(n * dtype.itemsize, POISON, dtype=np.uint8).view(dtype)


def expected_image(col, jobs, total):
    exp = poisoned(col.dtype, total)
    for s, st, c, o in jobs:
        exp[o:o + c] = col.expect[s][st:st + c]
    return exp


def report(col, jobs, got, exp):
    """The first job whose range (or the gap before it) differs: names width, start, count and alignment."""
    prev = 0
    for s, st, c, o in jobs:
        if not np.array_equal(got[prev:o + c], exp[prev:o + c]):
            w = int(col.descs["width"][s])
            return "w=%d start=%d count=%d align=%d bit0=%d" % (w, st, c, o % col.k, st * w % 128)
        prev = o + c
    return "after the last range"


@gpu
@pytest.mark.parametrize("which", ["fast_path", "edges"])
def test_unpack_jobs_at_every_bit_phase(adac, gpu_ctx, column, which):
    col = column
    jobs, total = (fast_path_jobs if which == "fast_path" else edge_jobs)(col.counts, col.tile, col.k)
    recs = adac.jobs_from_descs([col.descs[s] for s, _, _, _ in jobs], [(st, c) for _, st, c, _ in jobs],
                                [o for _, _, _, o in jobs])
    exp = expected_image(col, jobs, total + 8)
    size = col.dtype.itemsize
    d_dst = gpu_ctx.alloc((total + 9) * size + 64)
    for shift in (0, 1):                   # the output pointer itself: 16-byte aligned, and off by one element
        d_dst.upload(np.full((total + 9) * size + 64, POISON, dtype=np.uint8))
        adac.unpack_jobs(gpu_ctx, col.dtype, recs, col.d_words, d_dst.ptr + shift * size)
        gpu_ctx.sync()
        raw = d_dst.download(np.uint8, (total + 9) * size).view(col.dtype)
        assert np.all(raw[:shift] == poisoned(col.dtype, 1)[0])
        got = raw[shift:shift + total + 8]
        assert np.array_equal(got, exp), (col.dtype.name, which, shift, report(col, jobs, got, exp))
    d_dst.free()


@gpu
def test_unpack_range_at_every_bit_phase(adac, gpu_ctx, column):
    col = column
    cases, total = range_cases(col.counts, col.tile, col.k)
    exp = expected_image(col, cases, total + 8)
    d_dst = gpu_ctx.alloc((total + 8) * col.dtype.itemsize + 64)
    d_dst.upload(np.full((total + 8) * col.dtype.itemsize + 64, POISON, dtype=np.uint8))
    for s, st, c, o in cases:
        col.lay.unpack_range(col.d_words, s, st, c, d_dst, o)
    gpu_ctx.sync()
    got = d_dst.download(col.dtype, total + 8)
    assert np.array_equal(got, exp), (col.dtype.name, report(col, cases, got, exp))
    d_dst.free()


@gpu
def test_fetch_rows_at_every_bit_phase(adac, gpu_ctx, column):
    """Rows 0..127 cover every bit & 63 phase of a width (and with it every two-word straddle, off + w > 64); the last
    64 rows reach the segment's final word."""
    col = column
    n = int(col.counts[0])
    rows = np.concatenate([np.arange(128), np.arange(n - 64, n)]).astype(np.uint32)
    d_rows = gpu_ctx.upload(rows)
    d_out = gpu_ctx.alloc(len(rows) * col.dtype.itemsize + 16)
    for s in range(len(col.counts)):
        w = int(col.descs["width"][s])
        if w < 64 and 64 % w:
            assert ((rows.astype(np.uint64) * w) % 64 + w > 64).any()        # the batch does straddle two words
        d_segs = gpu_ctx.upload(np.full(len(rows), s, dtype=np.uint32))
        d_out.upload(poisoned(col.dtype, len(rows)))
        col.lay.fetch_rows(col.d_words, d_segs, d_rows, len(rows), d_out)
        got = d_out.download(col.dtype, len(rows))
        assert np.array_equal(got, col.expect[s][rows]), (col.dtype.name, w, np.flatnonzero(got != col.expect[s][rows])[:8])
        d_segs.free()
    # one call over segments of every width, in an order that mixes them
    rng = np.random.default_rng(17)
    segs = np.repeat(np.arange(len(col.counts)), len(rows)).astype(np.uint32)
    allrows = np.tile(rows, len(col.counts))
    order = rng.permutation(len(segs))
    segs, allrows = segs[order], allrows[order]
    d_mixed = gpu_ctx.alloc(len(segs) * col.dtype.itemsize + 16)
    d_mixed.upload(poisoned(col.dtype, len(segs)))
    d_s, d_r = gpu_ctx.upload(segs), gpu_ctx.upload(allrows)
    col.lay.fetch_rows(col.d_words, d_s, d_r, len(segs), d_mixed)
    got = d_mixed.download(col.dtype, len(segs))
    exp = np.stack(col.expect)[segs, allrows]
    assert np.array_equal(got, exp), (col.dtype.name, np.flatnonzero(got != exp)[:8])
    for b in (d_rows, d_out, d_mixed, d_s, d_r):
        b.free()
