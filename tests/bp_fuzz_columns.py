"""Column generators of the BITPACKING fuzz tests (host side only: numpy and the oracle, no GPU).

random_column is the generator of tests/test_gpu_bitpacking_fuzz.py and tools/soak_bitpacking.py: parts of random
lengths, a kind per part, built to reach the decision edges of BitpackingState::Flush.

edge_column builds a column from a SCHEDULE instead: one part per 2048-row metadata group, its kind taken from a list,
so that a pair of columns walks through every (mode of a, mode of b) combination and an 8-byte column reaches DELTA_FOR
at the widths between the one-dword prefix (w <= 26) and the wide field read (w > 32).  single_case / pair_case draw
everything one seed of tests/test_gpu_bitpacking_scans_fuzz.py runs - the columns, the placement, the masks, the range
probes, the key column - from one generator in a fixed order, so tests/test_bp_fuzz_census.py sees on the CPU exactly
what the GPU test scans."""
import numpy as np

from bp_decision_cases import lim
from oracle import bitpacking as bp

ALL = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
M64 = (1 << 64) - 1
GROUP = 2048


def _u(x):
    return np.uint64(int(x) & M64)


def _rand_int(rng, lo, hi):
    """uniform in [lo, hi] for Python ints spanning up to 2^64 values"""
    return lo + int(rng.integers(0, hi - lo, endpoint=True, dtype=np.uint64))


def _part(rng, dtype, m, kind):
    """m values of one pattern, as uint64 bit patterns (two's complement; narrower types keep the low bits)"""
    bits, ms, tmin, tmax = lim(dtype)
    sg = np.dtype(dtype).kind == "i"
    idx = np.arange(m, dtype=np.uint64)
    edge = [tmin, tmax, tmin + 1, tmax - 1, ms, ms + 1 if not sg else -1, 0]
    if kind == 0:                                   # constant, often at an edge
        x = edge[int(rng.integers(0, len(edge)))] if rng.random() < 0.5 else _rand_int(rng, tmin, tmax)
        return np.full(m, _u(x), dtype=np.uint64)
    if kind == 1:                                   # arithmetic run, either sign, may wrap
        step = int(rng.integers(-7, 8)) * (1 if rng.random() < 0.7 else int(rng.integers(1, 1 << (bits - 8) + 1)))
        total = step * (m - 1)
        if rng.random() < 0.3 or not tmin <= tmin - min(total, 0) <= tmax - max(total, 0):
            return _u(_rand_int(rng, tmin, tmax)) + _u(step) * idx
        return _u(_rand_int(rng, tmin - min(total, 0), tmax - max(total, 0))) + _u(step) * idx
    if kind == 2:                                   # sorted run, ascending or descending, mostly within range
        kk = int(rng.integers(0, min(bits - 2, 24) + 1))
        if rng.random() < 0.7:
            kk = min(kk, max(0, bits - 13))
        c = np.cumsum(rng.integers(0, 1 << kk, size=m, dtype=np.uint64), dtype=np.uint64)
        total = int(c[-1])
        desc = rng.random() < 0.5
        if rng.random() < 0.7 and total <= tmax - tmin:
            v0 = _rand_int(rng, tmin + total, tmax) if desc else _rand_int(rng, tmin, tmax - total)
        else:
            v0 = _rand_int(rng, tmin, tmax)
        return _u(v0) - c if desc else _u(v0) + c
    if kind == 3:                                   # random span of w bits anywhere in range, w up to B
        w = int(rng.integers(0, bits + 1))
        span = min((1 << w) - 1, tmax - tmin)
        lo = _rand_int(rng, tmin, tmax - span)
        v = _u(lo) + rng.integers(0, span, endpoint=True, size=m, dtype=np.uint64)
        if m > 2:
            v[0], v[m - 1] = _u(lo), _u(lo + span)
        return v
    if kind == 4:                                   # next to MIN / MAX
        r = int(rng.integers(0, bits))
        off = rng.integers(0, 1 << r, size=m, dtype=np.uint64)
        return _u(tmin) + off if rng.random() < 0.5 else _u(tmax) - off
    if kind == 5:                                   # unsigned: straddle T_S max; signed: span exactly T_S max
        if not sg:
            d = int(rng.integers(0, 200))
            return _u(ms - d) + (idx if rng.random() < 0.5 else rng.integers(0, 2 * d + 2, size=m, dtype=np.uint64))
        lo = _rand_int(rng, tmin, tmax - ms)
        v = _u(lo) + rng.integers(0, ms, endpoint=True, size=m, dtype=np.uint64)
        if m > 2:
            v[1], v[m - 1] = _u(lo), _u(lo + ms)
        return v
    if kind == 6:                                   # a ramp whose span crosses T_S max with narrow deltas
        step = ((tmax - tmin) // max(m, 1)) * int(rng.integers(5, 10)) // 10
        kk = int(rng.integers(0, 6))
        c = np.cumsum(rng.integers(0, 1 << kk, size=m, dtype=np.uint64), dtype=np.uint64)
        return _u(tmin + int(rng.integers(0, 1 << 8))) + _u(step) * idx + c
    return rng.integers(0, (1 << bits) - 1, endpoint=True, size=m, dtype=np.uint64)   # whole range


def random_column(rng):
    """(values, validity or None, force mode)"""
    dtype = np.dtype(ALL[int(rng.integers(0, len(ALL)))])
    ts = dtype.itemsize
    multi = rng.random() < 0.06
    if multi:   # wide random groups over more than two 256 KiB blocks
        n = int(2.3 * 262144 / ts) + int(rng.integers(0, 5000))
    else:
        n = int(rng.choice([1, 2, 3, 2047, 2048, 2049, 4095, 4097, int(rng.integers(1, 9000)),
                            int(rng.integers(9000, 30000))]))
    parts, left = [], n
    while left > 0:
        m = min(left, int(rng.choice([2048, 2048, 4096, int(rng.integers(1, 5000))])))
        kind = 7 if multi else int(rng.integers(0, 8))
        parts.append(_part(rng, dtype, m, kind))
        left -= m
    v = np.concatenate(parts)[:n].astype(np.dtype("u%d" % ts)).view(dtype)
    valid = None
    if rng.random() < 0.3:
        valid = rng.random(n) > rng.random() * 0.7
        if rng.random() < 0.4 and n > 2048:
            g = int(rng.integers(0, (n + 2047) // 2048))
            valid[g * 2048:(g + 1) * 2048] = False
    force = int(rng.integers(1, 5)) if rng.random() < 0.2 else 0
    return v, valid, force


# ---- the schedule-driven generator ---------------------------------------------------------------------------------
WIDE_DELTA, MIXED = 8, 9        # the kinds edge_column adds to _part's eight
MAX_DRAWS = 9                   # a refused column is redrawn at most 8 times; the ninth refusal fails the test
PART_DRAWS = 64                 # a part the codec refuses on its own is drawn again (most mixed signed ones are)
FIXED_N = [1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 4095, 4097]


def _as_type(bits64, dtype):
    dtype = np.dtype(dtype)
    return bits64.astype(np.dtype("u%d" % dtype.itemsize)).view(dtype)


def _wide_delta(rng, dtype, m):
    """8-byte types: a cumulative sum of fields below 2^k, k in 20 .. 40, ascending or descending; in some groups every
    field of one whole 64-row step (aligned to the step) is 2^k - 1, the largest sum a step's prefix can reach."""
    # k in 20 .. 40, two in five next to the one-dword prefix's bound (26 | 27) / the wide field read's (32 | 33)
    k = int(rng.choice([26, 27, 28, 31, 32, 33])) if rng.random() < 0.4 else int(rng.integers(20, 41))
    f = rng.integers(0, 1 << k, size=m, dtype=np.uint64)
    if m >= 128 and rng.random() < 0.5:
        s = 64 * int(rng.integers(1, m // 64))
        f[s:s + 64] = (1 << k) - 1            # field i is value i - value i-1: rows s .. s+63 are one step of the scan
    c = np.cumsum(f, dtype=np.uint64)         # < 2^51
    v0 = _rand_int(rng, 1 << 52, 1 << 62) * (-1 if np.dtype(dtype).kind == "i" and rng.random() < 0.5 else 1)
    return _u(v0) - c if rng.random() < 0.5 else _u(v0) + c


def _edge_part(rng, dtype, m, kind):
    dtype = np.dtype(dtype)
    if kind == WIDE_DELTA:
        return _wide_delta(rng, dtype, m) if dtype.itemsize == 8 else _part(rng, dtype, m, 2)
    if kind == MIXED:
        cut = int(rng.integers(0, m + 1))
        k1, k2 = (int(x) for x in rng.integers(0, 7 if dtype.kind == "i" else 8, size=2))
        return np.concatenate([_part(rng, dtype, cut, k1), _part(rng, dtype, m - cut, k2)]) if 0 < cut < m \
            else _part(rng, dtype, m, k1)
    return _part(rng, dtype, m, kind)


def _encodable_part(rng, dtype, m, kind):
    """One part the codec takes on its own: a single part it refuses (a signed run that wraps, a signed span wider
    than T_S) would make every column of a long schedule unencodable, so such a part is drawn again here; the
    refusals that depend on the whole column (its NULL mask, its forced mode) are left to the caller's redraw."""
    for i in range(PART_DRAWS):
        # (2048 rows of an int8 run with a step wrap whatever the start: after 16 draws the part is a random span)
        part = _edge_part(rng, dtype, m, kind if i < 16 else 3)
        try:
            bp.Compressed(_as_type(part, dtype))
            return part
        except ValueError:
            continue
    raise AssertionError("%d draws of kind %d refused for %s" % (PART_DRAWS, kind, np.dtype(dtype).name))


def edge_column(rng, dtype, n, kinds, validity=None, force=bp.MODE_AUTO):
    """n rows of `dtype`, group g (2048 rows) one part of kind kinds[g]; compressed as the decode fuzz does it.
    Returns (values, Compressed); ValueError when the codec refuses the column."""
    parts = [_encodable_part(rng, dtype, min(GROUP, n - g * GROUP), kinds[g]) for g in range((n + GROUP - 1) // GROUP)]
    v = _as_type(np.concatenate(parts), dtype)
    return v, bp.Compressed(v, validity, force, null_zero=validity is not None)


def _validity(rng, n):
    """a NULL mask on 0.3 of the draws, an all-NULL group now and then"""
    if rng.random() >= 0.3:
        return None
    valid = rng.random(n) > rng.random() * 0.7
    if rng.random() < 0.4:
        g = int(rng.integers(0, (n + GROUP - 1) // GROUP))
        valid[g * GROUP:(g + 1) * GROUP] = False
    return valid


class EdgeColumn:
    def __init__(self, values, validity, force, comp, draws):
        self.values, self.validity, self.force, self.comp, self.draws = values, validity, force, comp, draws
        self.dtype = values.dtype


def draw_column(rng, dtype, n, kinds):
    """edge_column with a validity (p = 0.3) and a forced mode (p = 0.2) drawn per attempt; redrawn while refused"""
    for draws in range(1, MAX_DRAWS + 1):
        validity = _validity(rng, n)
        force = int(rng.integers(1, 5)) if rng.random() < 0.2 else bp.MODE_AUTO
        try:
            v, comp = edge_column(rng, dtype, n, kinds, validity, force)
            return EdgeColumn(v, validity, force, comp, draws)
        except ValueError:
            continue
    raise AssertionError("nine draws refused: %s, %d rows" % (np.dtype(dtype).name, n))


# kinds by the mode they aim at (the codec decides; the census counts what was reached)
_TARGET = {bp.MODE_CONSTANT: [0], bp.MODE_CONSTANT_DELTA: [1], bp.MODE_DELTA_FOR: [2, 2, WIDE_DELTA, WIDE_DELTA],
           bp.MODE_FOR: [3, 4, 5, 7, MIXED, 6]}


def _kind_for(rng, target, dtype):
    opts = _TARGET[target]
    kind = opts[int(rng.integers(0, len(opts)))]
    if kind == WIDE_DELTA and np.dtype(dtype).itemsize != 8:
        kind = 2
    if kind == 7 and np.dtype(dtype).kind == "i":
        kind = 5                      # the whole range of a signed type is never encodable: its widest FOR span
    return kind


def _length(rng, seed):
    """the fixed lengths and the three random ones in turn with the seed, so 14 seeds in a row reach every one"""
    opts = FIXED_N + [int(rng.integers(1, 9000)), int(rng.integers(9000, 30000)), int(rng.integers(30000, 80000))]
    return opts[seed % len(opts)]


def seed_masks(rng, n, phase, validities):
    """The selection masks of one seed, as bools over nwords * 64 elements: name -> mask (None: no mask).  Elements no
    row covers - below the phase and past the span - hold random junk: it must change nothing."""
    span = phase + n
    size = (span + 63) // 64 * 64
    rows = slice(phase, span)

    def mask_of(row_bits):
        m = rng.random(size) < 0.5
        m[rows] = row_bits
        return m

    steps = np.repeat(rng.random((n + 63) // 64) < 0.5, 64)[:n]       # whole 64-row steps clear, from the first row
    one = np.zeros(n, dtype=bool)
    one[int(rng.integers(0, n))] = True
    masks = {"none": None, "random": mask_of(rng.random(n) < float(rng.choice([0.02, 0.5, 0.98]))),
             "steps": mask_of(steps), "one_bit": mask_of(one)}
    for name, valid in validities:
        if valid is not None:
            masks["validity_" + name] = mask_of(valid)
    return masks


class Case:
    pass


def _draw_type(rng):
    """the eight types, the two 8-byte ones twice as likely: only they have the one-dword / wide split of DELTA_FOR"""
    return np.dtype((ALL + ALL[6:])[int(rng.integers(0, len(ALL) + 2))])


def single_case(seed):
    """One single-column seed: a column of a random type and per-group kinds, its placement, masks and range probes."""
    rng = np.random.default_rng(seed)
    c = Case()
    c.seed = seed
    dtype = _draw_type(rng)
    c.n = _length(rng, seed)
    ngr = (c.n + GROUP - 1) // GROUP
    targets = rng.choice(CYCLE, size=ngr)
    c.col = draw_column(rng, dtype, c.n, [_kind_for(rng, int(t), dtype) for t in targets])
    c.phase = int(rng.integers(1, 131)) if rng.random() < 0.5 else 0
    c.one_cu = rng.random() < 0.25
    c.masks = seed_masks(rng, c.n, c.phase, [("a", c.col.validity)])
    info = np.iinfo(dtype)
    v = c.col.values
    draw = lambda: int(v[int(rng.integers(0, c.n))])  # noqa: E731
    x, y, z = draw(), draw(), draw()
    c.probes = [(int(info.min), int(info.max)), (min(x, y), max(x, y)), (z, z), (int(info.min), draw()),
                (draw(), int(info.max))]
    lo = draw()
    c.probes.append((lo, lo - 1) if lo > info.min else (int(info.min) + 1, int(info.min)))    # lo > hi
    if dtype.kind == "i":
        c.probes.append((-int(rng.integers(1, 1 << (dtype.itemsize * 8 - 2))),
                         int(rng.integers(0, 1 << (dtype.itemsize * 8 - 2)))))
    c.probes += interval_probes(rng, c.col)
    return c


def interval_probes(rng, col):
    """Ranges that end on, one inside and one outside the edges of one FOR group's interval [frame, frame + 2^w - 1]:
    where the range scans decide from the header alone that a group lies inside or outside the range."""
    info = np.iinfo(col.dtype)
    bits = 8 * col.dtype.itemsize
    fors = [g for g in segment_groups(col.comp) if g[3] == bp.MODE_FOR and g[4] >= 1]
    if not fors:
        return []
    _, _, _, _, w, frame, _ = fors[int(rng.integers(0, len(fors)))]
    lo = frame - (1 << bits) if col.dtype.kind == "i" and frame >> (bits - 1) else frame
    hi = lo + (1 << w) - 1                  # past T's maximum: the interval wraps and the scan walks the rows
    tmin, tmax = int(info.min), int(info.max)
    clamp = lambda x: min(max(x, tmin), tmax)  # noqa: E731
    return [(clamp(hi), clamp(hi)), (lo, lo), (clamp(hi), tmax), (tmin, lo), (clamp(hi + 1), tmax),
            (tmin, clamp(lo - 1)), (lo, clamp(hi)), (clamp(lo + 1), clamp(hi)), (lo, clamp(hi - 1))]


NGROUPS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256]
KEY_TYPES = [np.uint8, np.uint16, np.uint32, np.int8, np.uint64]


def key_column(rng, n, ngroups, ktype):
    """Keys in 0 .. ngroups + 2 (as far as the type holds them), one shape per 2048-row group: constant, ramp up or
    down (CONSTANT_DELTA, the second with a negative step), sorted walk ascending or descending (DELTA_FOR), random
    (FOR).  A ramp over more rows than there are keys runs on past ngroups + 2 where the type is wide enough - those
    rows belong in the overflow entry - and is a sorted walk where it is not."""
    ktype = np.dtype(ktype)
    top = min(ngroups + 2, int(np.iinfo(ktype).max), 120 if ktype.kind == "i" else 1 << 62)
    parts = []
    for g in range((n + GROUP - 1) // GROUP):
        m = min(GROUP, n - g * GROUP)
        shape = int(rng.integers(0, 6))
        if shape in (1, 2) and m - 1 > top and ktype.itemsize == 1:
            shape += 2
        if shape == 0:
            k = np.full(m, int(rng.integers(0, top + 1)), dtype=np.int64)
        elif shape in (1, 2):
            lo = int(rng.integers(0, max(top - (m - 1), 0) + 1))
            k = lo + np.arange(m, dtype=np.int64)
            k = k[::-1] if shape == 2 else k
        elif shape in (3, 4):
            k = np.sort(rng.integers(0, top + 1, size=m)).astype(np.int64)
            k = k[::-1] if shape == 4 else k
        else:
            k = rng.integers(0, top + 1, size=m).astype(np.int64)
            if ktype.kind == "i" and rng.random() < 0.5:
                k[rng.random(m) < 0.1] = -3         # a negative key is a large unsigned number of its own width
        parts.append(k)
    return np.concatenate(parts).astype(ktype)


# the targets one cycle walks, in an order drawn per seed: the two delta modes twice, as they are the ones a NULL
# mask, a narrow type or a value above T_S's maximum turns into FOR
CYCLE = [bp.MODE_CONSTANT, bp.MODE_CONSTANT_DELTA, bp.MODE_DELTA_FOR, bp.MODE_FOR, bp.MODE_CONSTANT_DELTA,
         bp.MODE_DELTA_FOR]
MULTI_EVERY, MULTI_AT = 12, 5     # pair seeds with seed % 12 == 5: segment counts that differ


def pair_case(seed):
    """One pair seed: two columns of the same length and independent types whose kinds walk the mode combinations
    (a's target cycles with the group index, b's with the group index divided by the cycle length), the shared
    placement, the masks, and the grouped call's key column and group count."""
    rng = np.random.default_rng(seed)
    c = Case()
    c.seed = seed
    c.multi = seed % MULTI_EVERY == MULTI_AT
    if c.multi:     # two-and-a-bit blocks of whole-range 8-byte values against a 1-byte column
        ta, tb = np.dtype(np.uint64), np.dtype([np.uint8, np.int8][int(rng.integers(0, 2))])
        c.n = int(2.3 * 262144 / 8) + int(rng.integers(0, 4000))
    else:
        ta, tb = _draw_type(rng), _draw_type(rng)
        c.n = _length(rng, seed)
    ngr = (c.n + GROUP - 1) // GROUP
    cyc = [int(t) for t in rng.permutation(CYCLE)]
    L = len(cyc)
    ra, rb = (int(x) for x in rng.integers(0, L, size=2))
    kinds_a = [7] * ngr if c.multi else [_kind_for(rng, cyc[(g + ra) % L], ta) for g in range(ngr)]
    kinds_b = [_kind_for(rng, cyc[(g // L + rb) % L], tb) for g in range(ngr)]
    c.a = draw_column(rng, ta, c.n, kinds_a)
    c.b = draw_column(rng, tb, c.n, kinds_b)
    c.phase = int(rng.integers(1, 131)) if rng.random() < 0.5 else 0
    c.one_cu = rng.random() < 0.25
    c.masks = seed_masks(rng, c.n, c.phase, [("a", c.a.validity), ("b", c.b.validity)])
    c.ngroups = NGROUPS[int(rng.integers(0, len(NGROUPS)))]
    c.b_is_key = rng.random() < 0.25
    c.ktype = np.dtype(KEY_TYPES[int(rng.integers(0, len(KEY_TYPES)))])
    c.keys = key_column(rng, c.n, c.ngroups, c.ktype)
    return c


def pair_columns(seed):
    """the two columns of a pair seed"""
    c = pair_case(seed)
    return c.a, c.b


SINGLE_SEEDS = [71_000 + i for i in range(96)]
PAIR_SEEDS = [72_000 + i for i in range(160)]


def segment_groups(comp):
    """Every metadata group of a Compressed column, read from the block images: (segment, group in the segment, rows,
    mode, width, frame, extra) - frame and extra as unsigned bit patterns of the column type.  CONSTANT: frame = the
    value.  CONSTANT_DELTA: frame = the first value, extra = the step.  FOR: the frame of reference.  DELTA_FOR:
    frame = the smallest delta, extra = the first value less that delta."""
    ts = comp.dtype.itemsize
    ut = np.dtype("u%d" % ts)
    out = []
    for i in range(comp.nseg):
        blk, rows = comp.block(i), comp.count(i)
        first = int(blk[:8].view(np.uint64)[0])
        for g in range((rows + GROUP - 1) // GROUP):
            enc = int(blk[first - 4 * (g + 1):first - 4 * g].view(np.uint32)[0])
            mode, off = enc >> 24, enc & 0xffffff
            word = lambda j: int(blk[off + j * ts:off + (j + 1) * ts].view(ut)[0])  # noqa: E731
            width = word(1) & 0xff if mode in (bp.MODE_FOR, bp.MODE_DELTA_FOR) else 0
            extra = word(1) if mode == bp.MODE_CONSTANT_DELTA else word(2) if mode == bp.MODE_DELTA_FOR else 0
            out.append((i, g, min(GROUP, rows - g * GROUP), mode, width, word(0), extra))
    return out
