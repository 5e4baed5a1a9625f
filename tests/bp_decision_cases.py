"""Decision table of the BITPACKING compressor, pinned by hand from the reference's rules.

Every row is a small column (one to three 2048-row metadata groups) with the mode and width that
`BitpackingState::Flush` must give each group, written down from the reference source and not from this
project's oracle: the oracle and the device planner share their arithmetic, so comparing one with the other
cannot find a mistake they both make.  Citations are relative to the reference checkout:

  bp.cpp    src/storage/compression/bitpacking.cpp
  bp.hpp    src/include/duckdb/common/bitpacking.hpp
  sub.cpp   src/function/scalar/operators/subtract.cpp

Rules used below (T the column type, T_S its signed twin, B = 8 * sizeof(T), M = NumericLimits<T_S>::Maximum()):
  CONSTANT        all rows NULL, or max == min, under AUTO / CONSTANT                     bp.cpp:225
  FOR allowed     TrySubtract<T>(max, min) succeeds                                       bp.cpp:148
  no delta        unsigned max > M (bp.cpp:154), fewer than 2 rows (:159), a NULL (:168), a delta outside T_S
                  when max - min does not fit T_S (:177-193), max_delta - min_delta outside T_S (:207),
                  row0 - min_delta outside T_S (:208-209)
  CONSTANT_DELTA  max_delta == min_delta, unless forced FOR / DELTA_FOR                   bp.cpp:235
  DELTA_FOR       MinimumBitWidth<T_U>(max_delta - min_delta) < MinimumBitWidth(min_max_diff), unless forced FOR
                  (bp.cpp:244-247).  min_max_diff is read even when the FOR subtraction failed: for int64 the
                  subtraction is __builtin_sub_overflow, which leaves the wrapped difference behind (sub.cpp:141-146);
                  for int8/16/32 OverflowCheckedSubtract leaves it untouched (sub.cpp:82-92), so it stays 0 (Reset).
  FOR width       MinimumBitWidth<T_U>(max - min)                                         bp.cpp:264
  widths          signed: 1 + bits of |x|, B for T's minimum (bp.hpp:138-161); unsigned: bits of x;
                  then GetEffectiveWidth: w + sizeof(T) > B -> B (bp.hpp:219-226)
  refused         none of the above: Flush returns false                                  bp.cpp:276

Also here: a restatement of the block placement rule (ReserveSpace / FlushAndCreateSegmentIfFull / FlushSegment,
bp.cpp:441-451,491-509) and the column shapes that fill a block exactly or miss by one byte.
"""
import numpy as np

AUTO, CONSTANT, CONSTANT_DELTA, DELTA_FOR, FOR = 0, 1, 2, 3, 4
MODES = (AUTO, CONSTANT, CONSTANT_DELTA, DELTA_FOR, FOR)
REFUSED = None
GROUP = 2048
BLOCK_SIZE = 262144 - 8

UNSIGNED = [np.uint8, np.uint16, np.uint32, np.uint64]
SIGNED = [np.int8, np.int16, np.int32, np.int64]
ALL = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]


def C():
    return (CONSTANT, 0)


def CD():
    return (CONSTANT_DELTA, 0)


def DF(w):
    return (DELTA_FOR, w)


def F(w):
    return (FOR, w)


def lim(dtype):
    """(B, M, T's min, T's max)"""
    dtype = np.dtype(dtype)
    bits = 8 * dtype.itemsize
    m = (1 << (bits - 1)) - 1
    return (bits, m, -m - 1, m) if dtype.kind == "i" else (bits, m, 0, (1 << bits) - 1)


def arr(vals, dtype):
    """Python ints -> dtype, wrapping modulo 2^B (so arithmetic runs that wrap are written as they wrap)."""
    dtype = np.dtype(dtype)
    mask = (1 << (8 * dtype.itemsize)) - 1
    u = np.array([int(x) & mask for x in vals], dtype=np.uint64)
    return u.astype(np.dtype("u%d" % dtype.itemsize)).view(dtype)


def scatter(n, lo, span, seed):
    """n values in [lo, lo + span], both ends present (rows 5 and 6)."""
    rng = np.random.default_rng(seed)
    x = [lo + int(r) for r in rng.integers(0, span, endpoint=True, size=n, dtype=np.uint64)]
    if n > 6:
        x[5], x[6] = lo, lo + span
    return x


def ramp(v0, deltas):
    out = [v0]
    for d in deltas:
        out.append(out[-1] + d)
    return out


class Case:
    def __init__(self, name, dtype, values, expect, cite, valid=None, force=AUTO):
        self.name, self.dtype, self.cite, self.force = name, np.dtype(dtype), cite, force
        self.values = arr(values, dtype)
        self.valid = None if valid is None else np.asarray(valid, dtype=bool)
        self.expect = expect   # list of (mode, width) per group, or REFUSED
        self.id = "%s-%s-%s" % (name, self.dtype.name, ["auto", "constant", "cdelta", "dfor", "for"][force])


def _cases():
    out = []
    add = out.append

    for dt in SIGNED:
        bits, m, tmin, tmax = lim(dt)
        lo = -(1 << (bits - 2)) - 3
        # span exactly M: FOR fits (sub.cpp:82-92 / :141).  Deltas +M and -M: max_delta - min_delta = 2M overflows
        # T_S (bp.cpp:207).  FOR width = bits(M) = B - 1 -> effective width B (bp.hpp:219-226), but int8 keeps 7
        # (7 + 1 is not above 8).
        v = scatter(GROUP, lo, m, 11)
        v[5], v[6], v[7] = lo, lo + m, lo
        add(Case("for_span_ts_max", dt, v, [F(7 if bits == 8 else bits)], "sub.cpp:82-92,141-146; bp.cpp:148,207,264; bp.hpp:219"))
        # span M + 1: FOR overflows (bp.cpp:148); max - min does not fit T_S so deltas are checked one by one, and
        # +(M+1) fails (bp.cpp:186-193): refused (bp.cpp:276), for every force mode.
        v = scatter(GROUP, lo, m + 1, 12)
        v[5], v[6], v[7] = lo, lo + m + 1, lo
        for fm in MODES:
            add(Case("for_span_ts_max_plus_1", dt, v, REFUSED, "bp.cpp:148,177-193,276", force=fm))

    # FOR overflows, deltas narrow.  v[i] = v0 + i * step + sum(inc[1..i]), inc in [0, 2^k - 1], both ends present:
    # max_delta - min_delta = 2^k - 1 -> delta width k.  max - min > M: FOR impossible (bp.cpp:148), every single delta
    # fits (bp.cpp:186-193), row0 - min_delta fits (bp.cpp:208-209).
    def narrow(v0, step, k, n=GROUP):
        inc = [(i * 7919) % (1 << k) for i in range(1, n)]
        inc[0], inc[1] = 0, (1 << k) - 1
        return ramp(v0, [step + x for x in inc])

    # int64: min_max_diff keeps the wrapped difference (sub.cpp:141-146), about -2^62 -> MinimumBitWidth = 64
    # (bp.hpp:138-161,219); delta width 20 < 64 -> DELTA_FOR (bp.cpp:244-247), also when forced CONSTANT,
    # CONSTANT_DELTA (max_delta != min_delta) or DELTA_FOR; forced FOR skips DELTA_FOR and FOR cannot hold it.
    v = narrow(-(3 << 61), 3 << 51, 20)
    for fm, exp in ((AUTO, [DF(20)]), (CONSTANT, [DF(20)]), (CONSTANT_DELTA, [DF(20)]), (DELTA_FOR, [DF(20)]),
                    (FOR, REFUSED)):
        add(Case("for_overflow_narrow_deltas", np.int64, v, exp, "sub.cpp:141-146; bp.cpp:148,245-247", force=fm))
    # int8/16/32: min_max_diff stays 0 (sub.cpp:82-92, bp.cpp:143) -> regular width 0, delta width is not below it:
    # refused (bp.cpp:247,263,276) under every force mode.
    narrow_small = {np.int32: narrow(-(3 << 29), 3 << 19, 2), np.int16: narrow(-(3 << 13), 24, 2),
                    np.int8: [-96 + (i * 192) // 2047 for i in range(GROUP)]}
    for dt, v in narrow_small.items():
        for fm in MODES:
            add(Case("for_overflow_narrow_deltas", dt, v, REFUSED, "sub.cpp:82-92,122-135; bp.cpp:143,247,276",
                     force=fm))

    # int64, the wrapped difference itself decides.  Deltas D + X, D + r, D, D, ...; span S = 2^64 - 2^54, so
    # min_max_diff wraps to -2^54: MinimumBitWidth = 1 + 55 = 56 (bp.hpp:150-161, 56 + 8 <= 64).  Delta width 55 < 56:
    # DELTA_FOR; delta width 56 is not below 56 and FOR overflows: refused.
    def wrapped(x_bits):
        s, x = (1 << 64) - (1 << 54), (1 << x_bits) - 1
        d = (s - x) // 2047
        r = (s - x) - 2047 * d
        return ramp(-(1 << 63) + d + 10, [d + x, d + r] + [d] * 2045)

    add(Case("wrapped_span_dw55", np.int64, wrapped(55), [DF(55)], "sub.cpp:141-146; bp.hpp:150-161; bp.cpp:245-247"))
    add(Case("wrapped_span_dw56", np.int64, wrapped(56), REFUSED, "sub.cpp:141-146; bp.hpp:219; bp.cpp:247,276"))

    for dt in SIGNED:
        bits, m, tmin, tmax = lim(dt)
        # row0 - min_delta below T_S's minimum (bp.cpp:208-209): no delta, FOR of span 118 -> width 7
        add(Case("delta_offset_overflows", dt, [tmin + 1 + 2 * i for i in range(60)], [F(7)], "bp.cpp:208-209,264"))
        add(Case("delta_offset_fits", dt, [tmin + 2 + 2 * i for i in range(60)], [CD()], "bp.cpp:208-209,235"))
        # descending from T's maximum: row0 - (-2) above M
        add(Case("delta_offset_overflows_desc", dt, [tmax - 1 - 2 * i for i in range(60)], [F(7)],
                 "bp.cpp:208-209,264"))
        add(Case("delta_offset_fits_desc", dt, [tmax - 2 - 2 * i for i in range(60)], [CD()], "bp.cpp:208-209,235"))
        # 0, a, 0, -b: span a + b fits, deltas +-a: max_delta - min_delta = 2a overflows T_S (bp.cpp:207) -> FOR.
        # span = 7 << (B - 4): bits B - 1 -> B except for int8 (7 + 1 <= 8 keeps 7)
        a, b = 5 << (bits - 4), 2 << (bits - 4)
        add(Case("delta_range_overflows", dt, [(0, a, 0, -b)[i % 4] for i in range(GROUP)],
                 [F(7 if bits == 8 else bits)], "bp.cpp:207,264; bp.hpp:219"))
        # can_do_all false (bp.cpp:177) and the one jump overflows T_S (bp.cpp:186-193): no delta, no FOR: refused
        add(Case("one_delta_overflows", dt, [tmin + 5] * 1024 + [tmax - 5] * 1024, REFUSED, "bp.cpp:177-193,276"))

    for dt in UNSIGNED:
        bits, m, tmin, tmax = lim(dt)
        # deltas +-a: 2a overflows T_S (bp.cpp:207) -> FOR of span a = 5 << (B - 4): bits B - 1
        a = 5 << (bits - 4)
        add(Case("delta_range_overflows", dt, [(0, a)[i % 2] for i in range(GROUP)], [F(7 if bits == 8 else bits)],
                 "bp.cpp:207,264; bp.hpp:219"))
        # maximum == M still allows deltas; M + 1 does not (bp.cpp:154).  Same arithmetic column shifted by one.
        n, step, w = (100, 1, 7) if bits == 8 else (GROUP, 3, 13)   # FOR width = bits((n - 1) * step)
        add(Case("unsigned_max_at_ts_max", dt, [m - (n - 1) * step + step * i for i in range(n)], [CD()],
                 "bp.cpp:154,235"))
        add(Case("unsigned_max_above_ts_max", dt, [m + 1 - (n - 1) * step + step * i for i in range(n)], [F(w)],
                 "bp.cpp:154,264"))
        # values far above M: no delta at all, FOR at the top of the range (span 100: width 7; 1000: width 10)
        span = 100 if bits == 8 else 1000
        add(Case("unsigned_top_of_range", dt, scatter(GROUP, tmax - span, span, 13), [F(7 if bits == 8 else 10)],
                 "bp.cpp:154,264"))
        # descending from M: row0 - (-step) = M + step overflows T_S (bp.cpp:208-209); from M - 2 it fits
        add(Case("delta_offset_overflows_desc", dt, [m - 1 - 2 * i for i in range(60)], [F(7)], "bp.cpp:208-209,264"))
        add(Case("delta_offset_fits_desc", dt, [m - 2 - 2 * i for i in range(60)], [CD()], "bp.cpp:208-209,235"))

    # descending DELTA_FOR (negative frame) and CONSTANT_DELTA with a negative step, every type.
    # 16-64 bit: deltas -(s + i % 8), i = 1..2047: sum(i % 8) = 7168, delta width bits(7) = 3 (bp.cpp:244).
    # span 2047 s + 7168; regular width (bp.cpp:245): unsigned bits(span), signed 1 + bits(span).
    # 8 bit: 100 rows, deltas -(i % 2): span 50, delta width 1; regular width u8 6, i8 7.
    for dt in ALL:
        bits, m, tmin, tmax = lim(dt)
        sg = np.dtype(dt).kind == "i"
        if bits == 8:
            deltas, v0 = [-(i % 2) for i in range(1, 100)], (20 if sg else 60)
            cstep, cn, c0 = -1, 100, (20 if sg else 120)
        elif bits == 16:
            deltas, v0 = [-(i % 8) for i in range(1, GROUP)], (3000 if sg else 7268)
            cstep, cn, c0 = -3, GROUP, (3000 if sg else 6200)
        else:
            deltas, v0 = [-(1000 + i % 8) for i in range(1, GROUP)], (1_000_000 if sg else 2_054_268)
            cstep, cn, c0 = -1000, GROUP, (1_000_000 if sg else 2_050_000)
        add(Case("descending_delta_for", dt, ramp(v0, deltas), [DF(1 if bits == 8 else 3)], "bp.cpp:244-247"))
        add(Case("constant_delta_negative_step", dt, [c0 + cstep * i for i in range(cn)], [CD()], "bp.cpp:235"))
        # forced FOR on the same descending column: FOR width unsigned bits(span) (bp.cpp:247,264):
        # 8 bit span 50 -> 6, 16 bit 7168 -> 13, 32/64 bit 2054168 -> 21
        add(Case("descending_delta_for", dt, ramp(v0, deltas), [F({8: 6, 16: 13}.get(bits, 21))], "bp.cpp:247,264",
                 force=FOR))

    # 8-bit arithmetic runs that wrap.  u8 (200 + 3i) mod 256 reaches 255 > M: no delta (bp.cpp:154), FOR over
    # [0, 255] = width 8.  i8 3i wraps across [-128, 127]: FOR overflows, the wrap delta -253 overflows: refused.
    add(Case("wrapping_run", np.uint8, [200 + 3 * i for i in range(GROUP)], [F(8)], "bp.cpp:154,264"))
    add(Case("wrapping_run", np.int8, [3 * i for i in range(GROUP)], REFUSED, "bp.cpp:148,186-193,276"))
    add(Case("wrapping_run_short", np.uint8, [250 + i for i in range(20)], [F(8)], "bp.cpp:154,264"))
    add(Case("wrapping_run_short", np.int8, [120 + i for i in range(20)], REFUSED, "bp.cpp:148,186-193,276"))

    # NULLs.  NULL slots hold T's extremes: they must not reach min / max (bp.cpp:285-289).
    for dt in ALL:
        bits, m, tmin, tmax = lim(dt)
        junk = [tmin, tmax]
        # group 0 constant 7, group 1 all NULL: CONSTANT under AUTO / CONSTANT (bp.cpp:225).  Forced otherwise the
        # all-NULL group keeps Reset's min = T max, max = T min: FOR subtraction fails, no delta: refused.
        v = [7] * GROUP + [junk[i % 2] for i in range(GROUP)]
        valid = [True] * GROUP + [False] * GROUP
        for fm, exp in ((AUTO, [C(), C()]), (CONSTANT, [C(), C()]), (CONSTANT_DELTA, REFUSED),
                        (DELTA_FOR, REFUSED), (FOR, REFUSED)):
            add(Case("all_null_group", dt, v, exp, "bp.cpp:131-145,148,168,225,276", valid=valid, force=fm))
        # one valid row, the rest NULL: max == min -> CONSTANT
        add(Case("one_valid_row", dt, [junk[i % 2] if i != 700 else 42 for i in range(GROUP)], [C()], "bp.cpp:225",
                 valid=[i == 700 for i in range(GROUP)]))
        # a NULL at the first or last row of an arithmetic run: no delta (bp.cpp:168), FOR of the valid rows' span:
        # 8 bit 10 + i over 100 rows -> span 98, width 7; otherwise 1000 + 3i over 2048 rows -> span 6138, width 13
        n, base, step, w = (100, 10, 1, 7) if bits == 8 else (GROUP, 1000, 3, 13)
        for row, j in ((0, tmax), (n - 1, tmin)):
            v = [base + step * i for i in range(n)]
            v[row] = j
            add(Case("null_at_row_%d" % (0 if row == 0 else 1), dt, v, [F(w)], "bp.cpp:168,264,285-289",
                     valid=[i != row for i in range(n)]))

    # Tails.  Group 0: 7 + i % 16: deltas +1 and -15, delta width bits(16) = 5, regular width unsigned 4, signed 5:
    # FOR width 4 (bp.cpp:247,264).  A 1-row tail is CONSTANT (bp.cpp:225); forced otherwise it is FOR width 0 (fewer
    # than 2 rows: no delta, bp.cpp:159).  A 2-row tail [3, 9] has one delta: CONSTANT_DELTA (bp.cpp:235); forced FOR:
    # width bits(6) = 3; forced DELTA_FOR: delta width 0 < regular width -> DELTA_FOR 0.
    for dt in ALL:
        g0 = [7 + i % 16 for i in range(GROUP)]
        add(Case("rows_2047", dt, g0[:2047], [F(4)], "bp.cpp:247,264"))
        for fm, e1, e2 in ((AUTO, C(), CD()), (CONSTANT, C(), CD()), (CONSTANT_DELTA, F(0), CD()),
                           (DELTA_FOR, F(0), DF(0)), (FOR, F(0), F(3))):
            add(Case("tail_1_row", dt, g0 + [3], [F(4), e1], "bp.cpp:159,225,264", force=fm))
            add(Case("tail_2_rows", dt, g0 + [3, 9], [F(4), e2], "bp.cpp:235,244-247,264", force=fm))
    return out


CASES = _cases()


def columns():
    """The table grouped by column: [(key, first case, {force mode: expectation})]."""
    out = {}
    for c in CASES:
        key = "%s-%s" % (c.name, c.dtype.name)
        first = out.setdefault(key, (key, c, {}))[1]
        assert np.array_equal(first.values, c.values) and first.force != c.force or first is c, c.id
        out[key][2][c.force] = c.expect
    return list(out.values())


# ---- block placement (ReserveSpace + FlushAndCreateSegmentIfFull + FlushSegment, bp.cpp:441-451,491-509) ----

def group_bytes(dtype, rows, mode, width):
    """data bytes of one group (BitpackingWriter, bp.cpp:374-437; GetRequiredSize, bp.hpp:99-102)"""
    ts = np.dtype(dtype).itemsize
    packed = (rows + 31) // 32 * 32 * width // 8
    return {CONSTANT: ts, CONSTANT_DELTA: 2 * ts, FOR: packed + 2 * ts, DELTA_FOR: packed + 3 * ts}[mode]


def place(dtype, groups):
    """groups: [(rows, mode, width)].  Returns (segments [(start, count, size)], slack) where slack[g] is the free
    space left when group g was placed: meta_ptr - data_ptr - (bytes + 4) in the block it went to, negative when the
    group did not fit the block it was offered first (it then opens a new one)."""
    segs, slack = [], []
    data, meta, start, count, k = 8, BLOCK_SIZE, 0, 0, 0

    def close():
        off = (data + 7) // 8 * 8
        segs.append((start, count, off + 4 * k))

    for rows, mode, width in groups:
        need = group_bytes(dtype, rows, mode, width) + 4
        s = meta - data - need
        if s < 0:
            close()
            start, count, k, data, meta = start + count, 0, 0, 8, BLOCK_SIZE
        slack.append(s)
        data += need - 4
        meta -= 4
        count += rows
        k += 1
    close()
    return segs, slack


def fill_shape(dtype, short):
    """A column of CONSTANT groups, FOR groups of one wide width and one FOR group of a second width, whose block
    is filled exactly (short = 0: the last group leaves 0 bytes) or misses by `short` bytes, followed by one more
    FOR group.  Returns (values, groups [(rows, mode, width)], index of the boundary group)."""
    dtype = np.dtype(dtype)
    bits, m, tmin, tmax = lim(dtype)
    ts = dtype.itemsize
    wide = bits - 1 if bits == 8 else bits // 2
    widths = [w for w in range(1, bits + 1) if not (w + ts > bits and w != bits)]   # bp.hpp:219-226
    cost_c = ts + 4
    cost_f = {w: group_bytes(dtype, GROUP, FOR, w) + 4 for w in widths}
    target = BLOCK_SIZE - 8 + short
    best = None
    for a in range(target // cost_f[wide], -1, -1):
        for w2 in widths:
            rem = target - a * cost_f[wide] - cost_f[w2]
            if rem >= 0 and rem % cost_c == 0:
                best = (a, w2, rem // cost_c)
                break
        if best:
            break
    assert best, (dtype, short)
    a, w2, c = best
    groups = [(GROUP, CONSTANT, 0)] * c + [(GROUP, FOR, wide)] * a + [(GROUP, FOR, w2), (GROUP, FOR, wide)]
    vals = []
    for g, (_, mode, w) in enumerate(groups):
        if mode == CONSTANT:
            vals += [g % 5 + 1] * GROUP
            continue
        # random over a span of width w (the full width: T's whole range, or [T min, T min + M] when signed), with
        # the ends alternating at rows 7-10 so that the deltas span about twice the values: AUTO takes FOR
        if w == bits:
            lo, span = tmin, (m if dtype.kind == "i" else tmax)
        else:
            lo, span = (tmin + 3 if dtype.kind == "i" else 3), (1 << w) - 1
        v = scatter(GROUP, lo, span, 1000 + g)
        v[7], v[8], v[9], v[10] = lo, lo + span, lo, lo + span
        vals += v
    return arr(vals, dtype), groups, c + a


FILL_SHAPES = [(np.uint8, 0), (np.uint8, 1), (np.int8, 1), (np.int16, 0), (np.int16, 2), (np.uint32, 0),
               (np.int64, 0), (np.uint64, 4)]


# ---- width sweeps under forced modes ----

def eff(dtype, w):
    """GetEffectiveWidth (bp.hpp:219-226)"""
    dtype = np.dtype(dtype)
    return 8 * dtype.itemsize if w + dtype.itemsize > 8 * dtype.itemsize else w


def max_delta_width(dtype):
    """The widest DELTA_FOR group a type can hold: the delta width must stay below the regular width
    (bp.cpp:247) and below the GetEffectiveWidth jump; uint8 values stay <= 127 (bp.cpp:154), so its regular width
    is at most 7."""
    dtype = np.dtype(dtype)
    return 6 if dtype == np.uint8 else 8 * dtype.itemsize - dtype.itemsize


def for_sweep(dtype, seed=0):
    """One 2048-row group per span width k (0 .. B, signed 0 .. B - 1), for forced FOR: width eff(k).  Even k sit
    at the top of T's range, odd k at the bottom."""
    dtype = np.dtype(dtype)
    bits, m, tmin, tmax = lim(dtype)
    vals, exp = [], []
    for k in range(0, bits + (0 if dtype.kind == "i" else 1)):
        span = (1 << k) - 1
        lo = tmax - span if k % 2 == 0 else tmin
        v = scatter(GROUP, lo, span, seed * 100 + k)
        vals += v
        exp.append(F(eff(dtype, k)))
    return arr(vals, dtype), exp


def delta_for_sweep(dtype, descending, seed=0):
    """One 2048-row group per delta width k (1 .. max_delta_width, then the first width past the GetEffectiveWidth
    jump for 16-64 bit types), then a 100-row group of constant step (delta width 0), for forced DELTA_FOR.
    Deltas are sign * inc with inc in [0, 2^k - 1] (rows 1 and 2 hold both ends); unsigned columns add one step of 1
    so that the regular width exceeds k.  Returns (values, expected (mode, width) per group)."""
    dtype = np.dtype(dtype)
    bits, m, tmin, tmax = lim(dtype)
    sg = dtype.kind == "i"
    rng = np.random.default_rng(seed)
    sign = -1 if descending else 1
    ks = list(range(1, max_delta_width(dtype) + 1)) + ([bits - dtype.itemsize + 1] if bits > 8 else [])
    vals, exp = [], []
    for k in ks:
        inc = [0] * (GROUP - 1)
        inc[1] = (1 << k) - 1
        if not sg:
            inc[2] = 1
        budget = max(0, min(64, ((1 << (bits - 2)) - (1 << k)) >> k))
        for r in rng.integers(4, GROUP - 1, size=budget):
            inc[int(r)] = int(rng.integers(0, 1 << k, dtype=np.uint64))
        span = sum(inc)
        if sg:
            v0 = -((span + 1) // 2) if not descending else 0
        else:
            v0 = 0 if not descending else span
        vals += ramp(v0, [sign * x for x in inc])
        exp.append(DF(k) if k <= max_delta_width(dtype) else F(eff(dtype, span.bit_length())))
    if sg:
        v0 = -50 if not descending else 0
    else:
        v0 = 0 if not descending else 99
    vals += [v0 + sign * i for i in range(100)]
    exp.append(DF(0))
    return arr(vals, dtype), exp
