"""adac_unpack through the tile table cut on 128-byte lines of the output (csrc/adac_tile_cut.h).

A segment that starts `ph` elements past a line is decoded as a head tile of TILE - ph rows and then whole tiles that
start on a line, so the full decode now stages images whose first field sits at any bit of a 16-byte chunk (bit0 != 0)
and runs the static full-tile path on segments that start at an odd element.  Every case decodes with adac_unpack,
compares with the input, and compares byte for byte with adac_unpack_range of each segment, whose tiles are still cut
relative to the range's first row."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

TILE_BYTES, LINE_BYTES = 16384, 128
SENTINEL = 0xA5
TYPES = [np.uint8, np.uint16, np.uint32, np.uint64, np.int32]
# passes over the count list per type size: each case stays at about 300 K rows or below
PASSES = {1: 2, 2: 4, 4: 6, 8: 6}


def geometry(dtype):
    size = np.dtype(dtype).itemsize
    return TILE_BYTES // size, LINE_BYTES // size, 16 // size


def phases_of(dtype):
    tile, line, k = geometry(dtype)
    return sorted({0, 1, k - 1, k, k + 1, line - 1})


def sizes_of(dtype):
    tile, line, k = geometry(dtype)
    return [1, k - 1, line - 1, line, tile - line, tile - 1, tile, tile + 1, tile + line - 1, 2 * tile, 2 * tile + 1]


def widths_of(dtype):
    tb = 8 * np.dtype(dtype).itemsize
    return [w for w in (1, 8, 31, 32, 33, 64) if w < tb] + [tb]        # tb: the segment stays unpacked, no min


def dense_counts(dtype):
    """Back-to-back segments whose start phases modulo the line follow phases_of(): a short filler segment (itself a
    case) moves the running sum to the wanted phase before every count of sizes_of(); one empty segment in the middle."""
    tile, line, k = geometry(dtype)
    sizes, phases = sizes_of(dtype), phases_of(dtype)
    counts, run = [], 0
    for ps in range(PASSES[np.dtype(dtype).itemsize]):
        for i, c in enumerate(sizes):
            fill = (phases[(i + ps) % len(phases)] - run) % line
            if fill:
                counts.append(fill)
                run += fill
            counts.append(c)
            run += c
            if ps == 0 and i == 5:
                counts.append(0)
    return np.array(counts, dtype=np.uint32)


def gapped_offsets(dtype, counts):
    """Explicit element offsets with gaps: segment j starts at phase phases[(j + 3) % len] of a line of its own."""
    tile, line, k = geometry(dtype)
    phases = phases_of(dtype)
    offs, at = [], 0
    for j, c in enumerate(counts):
        at = (at + 2 * line - 1) // line * line + phases[(j + 3) % len(phases)]
        offs.append(at)
        at += int(c)
    return np.array(offs, dtype=np.uint64)


def segment_values(rng, dtype, n, w):
    """n values whose range needs exactly w bits (n >= 2); w = 8 * sizeof(T): the whole range of T.  Signed types:
    packed segments lie below zero, so the frame of reference added back is negative."""
    dtype = np.dtype(dtype)
    tb = 8 * dtype.itemsize
    span = rng.integers(0, 2 ** w, size=n, dtype=np.uint64)
    if n >= 2:
        span[0], span[n - 1] = 0, 2 ** w - 1
    if w == tb:
        lo = 2 ** (tb - 1) if dtype.kind == "i" else 0                # bit pattern of T's smallest value
    elif dtype.kind == "i":
        lo = 2 ** tb - 2 ** w - min(7, 2 ** (tb - 1) - 2 ** w)         # [-2^w - 7, -8], or [-2^w, -1] at w = tb - 1
    else:
        lo = min(2 ** tb - 2 ** w, 2 ** w // 3 + 11)
    bits = (span + np.uint64(lo)) & np.uint64(2 ** tb - 1)
    return bits.astype(np.dtype("u%d" % dtype.itemsize)).view(dtype)


def column_values(dtype, counts, seed):
    rng = np.random.default_rng(seed)
    widths = widths_of(dtype)
    seg_w = [widths[j % len(widths)] for j in range(len(counts))]
    segs = [segment_values(rng, dtype, int(c), w) for c, w in zip(counts, seg_w)]
    return segs, seg_w


def start_offsets(counts):
    return np.concatenate([[0], np.cumsum(counts.astype(np.uint64))[:-1]]).astype(np.uint64)


@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
def test_lists_cover_the_phases_counts_and_widths(dtype):
    """Held on the CPU: what the GPU cases below rely on."""
    tile, line, k = geometry(dtype)
    counts = dense_counts(dtype)
    offs = start_offsets(counts)
    assert int(counts.sum()) <= 300_000
    live = counts > 0
    assert set((offs[live] % line).tolist()) >= set(phases_of(dtype))
    assert set(counts.tolist()) >= set(sizes_of(dtype))
    empty = np.flatnonzero(counts == 0)
    assert len(empty) == 1 and 0 < empty[0] < len(counts) - 1
    # every width meets a segment of more than one tile that starts off a line: a head tile and bit0 != 0 after it
    widths = widths_of(dtype)
    seen = {widths[j % len(widths)] for j in range(len(counts)) if counts[j] > tile and offs[j] % line}
    assert seen == set(widths), seen
    g = gapped_offsets(dtype, counts)
    assert np.all(g[1:] >= g[:-1] + counts[:-1]) and set((g % line).tolist()) >= set(phases_of(dtype))


class Column:
    pass


@pytest.fixture(scope="module", params=TYPES, ids=lambda t: np.dtype(t).name)
def column(request, adac, gpu_ctx):
    """One encoded column per type, shared by the cases below and left unchanged by them."""
    dtype = np.dtype(request.param)
    tile, line, k = geometry(dtype)
    assert adac.tile_values(dtype) == tile
    c = Column()
    c.dtype, c.counts = dtype, dense_counts(dtype)
    c.segs, c.seg_w = column_values(dtype, c.counts, 1700 + dtype.itemsize + (dtype.kind == "i"))
    c.vals = np.concatenate(c.segs)
    c.lay = adac.Layout(gpu_ctx, dtype, c.counts)
    d_vals = gpu_ctx.upload(c.vals)
    c.d_words = gpu_ctx.alloc(c.lay.max_arena_words * 8 + 16).zero()
    c.lay.encode(d_vals, c.d_words)
    gpu_ctx.sync()
    d_vals.free()
    c.descs = c.lay.get_descs()
    tb = 8 * dtype.itemsize
    for j, n in enumerate(c.counts):
        if n >= 2:
            assert int(c.descs["width"][j]) == c.seg_w[j], (j, int(n))
            assert bool(c.descs["flags"][j] & adac.SEG_PACKED) == (c.seg_w[j] < tb)
    yield c
    c.lay.close()
    c.d_words.free()


def sentinel_bytes(n):
    return np.full(n, SENTINEL, dtype=np.uint8)


def decode_both_ways(ctx, lay, d_words, dtype, counts, offs, span, shift_bytes=0):
    """adac_unpack, and adac_unpack_range of every segment, each into a buffer prefilled with the sentinel and handed in
    `shift_bytes` into its allocation: the two images as bytes, allocation pad included."""
    size = dtype.itemsize
    nbytes = shift_bytes + span * size + 256
    images = []
    for whole in (True, False):
        d_out = ctx.alloc(nbytes)
        assert d_out.ptr % LINE_BYTES == 0
        d_out.upload(sentinel_bytes(nbytes))
        if whole:
            lay.unpack(d_words, d_out.ptr + shift_bytes)
        else:
            for s, n in enumerate(counts):
                lay.unpack_range(d_words, s, 0, int(n), d_out.ptr + shift_bytes, int(offs[s]))
        ctx.sync()
        images.append(d_out.download(np.uint8, nbytes))
        d_out.free()
    return images


def expected_image(dtype, segs, offs, span, shift_bytes=0):
    size = dtype.itemsize
    exp = sentinel_bytes(shift_bytes + span * size + 256)
    body = exp[shift_bytes:shift_bytes + span * size].view(dtype)
    for v, o in zip(segs, offs):
        body[int(o):int(o) + len(v)] = v
    return exp


def first_difference(dtype, counts, offs, got, exp, shift_bytes=0):
    size = dtype.itemsize
    bad = np.flatnonzero(got != exp)
    if not len(bad):
        return None
    e = (int(bad[0]) - shift_bytes) // size
    s = int(np.searchsorted(offs, e, side="right")) - 1
    return "byte %d = element %d: segment %d (count %d, starts at element %d) row %d; %d bytes differ" % (
        bad[0], e, s, int(counts[s]), int(offs[s]), e - int(offs[s]), len(bad))


@gpu
def test_dense_segments_at_every_phase_count_and_width(gpu_ctx, column):
    col = column
    offs = start_offsets(col.counts)
    span = len(col.vals)
    whole, ranges = decode_both_ways(gpu_ctx, col.lay, col.d_words, col.dtype, col.counts, offs, span)
    exp = expected_image(col.dtype, col.segs, offs, span)
    assert np.array_equal(whole, exp), first_difference(col.dtype, col.counts, offs, whole, exp)
    assert np.array_equal(whole, ranges), first_difference(col.dtype, col.counts, offs, whole, ranges)


@gpu
def test_output_as_a_view_16_bytes_into_its_allocation(gpu_ctx, column):
    """Alignment is by element index: with the output 16 bytes off a line the same tiles store the same values."""
    col = column
    offs = start_offsets(col.counts)
    span = len(col.vals)
    whole, ranges = decode_both_ways(gpu_ctx, col.lay, col.d_words, col.dtype, col.counts, offs, span, shift_bytes=16)
    exp = expected_image(col.dtype, col.segs, offs, span, shift_bytes=16)
    assert np.array_equal(whole, exp), first_difference(col.dtype, col.counts, offs, whole, exp, 16)
    assert np.array_equal(whole, ranges)


@gpu
def test_gapped_value_offsets_leave_the_gaps_alone(adac, gpu_ctx, column):
    """The same packed words under explicit val_offs with gaps: every element outside the segments keeps the sentinel."""
    col = column
    offs = gapped_offsets(col.dtype, col.counts)
    lay = adac.Layout(gpu_ctx, col.dtype, col.counts, offs)
    descs = col.descs.copy()
    descs["val_off"] = offs
    lay.set_descs(descs)
    span = int(lay.value_span)
    assert span == int(offs[-1]) + int(col.counts[-1]) and span > len(col.vals)
    whole, ranges = decode_both_ways(gpu_ctx, lay, col.d_words, col.dtype, col.counts, offs, span)
    exp = expected_image(col.dtype, col.segs, offs, span)
    assert np.array_equal(whole, exp), first_difference(col.dtype, col.counts, offs, whole, exp)
    assert np.array_equal(whole, ranges)
    lay.close()


@gpu
def test_decode_records_knob_keeps_the_segment_relative_tiles(adac, gpu_ctx, column):
    """tile_records bit 1: the A/B form through the expanded records of the segment-relative table, same values."""
    col = column
    offs = start_offsets(col.counts)
    span = len(col.vals)
    adac.set_tuning("tile_records", 3)
    try:
        whole, _ = decode_both_ways(gpu_ctx, col.lay, col.d_words, col.dtype, col.counts[:0], offs, span)
    finally:
        adac.set_tuning("tile_records", 1)
    exp = expected_image(col.dtype, col.segs, offs, span)
    assert np.array_equal(whole, exp), first_difference(col.dtype, col.counts, offs, whole, exp)


@gpu
def test_first_flush_of_the_benchmark_layout(adac, gpu_ctx):
    """u64, the Appender's first flush: 8 segments, 204 800 rows, three of them starting at an odd element and only
    three on a line."""
    dtype = np.dtype(np.uint64)
    counts = adac.appender_segment_counts(204800, 8)
    assert counts.tolist() == [2048, 32767, 32767, 32767, 22531, 32767, 32767, 16386]
    offs = start_offsets(counts)
    assert int((offs % 2).sum()) == 3 and int((offs % 16 == 0).sum()) == 3
    rng = np.random.default_rng(42)
    vals = rng.integers(0, 2 ** 32, size=204800, dtype=np.uint64)
    vals[offs.astype(np.int64)] = 0
    vals[(offs + counts - 1).astype(np.int64)] = 2 ** 32 - 1                  # every segment at w = 32, like C2
    lay = adac.Layout(gpu_ctx, dtype, counts)
    d_vals = gpu_ctx.upload(vals)
    d_words = gpu_ctx.alloc(lay.max_arena_words * 8 + 16).zero()
    lay.encode(d_vals, d_words)
    gpu_ctx.sync()
    assert set(lay.get_descs()["width"].tolist()) == {32}
    segs = [vals[int(o):int(o) + int(n)] for o, n in zip(offs, counts)]
    whole, ranges = decode_both_ways(gpu_ctx, lay, d_words, dtype, counts, offs, len(vals))
    exp = expected_image(dtype, segs, offs, len(vals))
    assert np.array_equal(whole, exp), first_difference(dtype, counts, offs, whole, exp)
    assert np.array_equal(whole, ranges)
    lay.close()
    d_vals.free()
    d_words.free()
