"""Cases for the re-compaction kernels (adac_analyze_packed, adac_repack, adac_reencode): a mirror of the predicates by
which k_analyze_packed_g and k_repack_g (csrc/adac_kernels.hip) choose their form, and the generator of the
(old_w, new_w) plane that tests/test_gpu_repack_matrix.py runs.  No GPU and no library is needed to import this:
tests/test_repack_census.py asserts on the CPU what the generated columns reach.

A column of the plane holds one segment per pair (old_w, new_w) in 1..tb x 1..tb (tb = bits of the type).  The segment is
first encoded from WIDE values that give it a frame of exactly old_w bits (old_w = tb: an unpacked source), then its
rows are rewritten in place, at the old width and min, with NARROW values.  What the pair's new_w means depends on the
call: adac_repack is handed a destination descriptor of exactly (new_w, dst min); adac_reencode finds the width itself,
which is the number of bits the narrow values need ("bits" below: min(old_w, new_w), one less on every third pair).

Rotations (all exact, asserted by the census):
  size      (old_w + new_w) % 4      -> 3 rows, 129 rows, one tile, two tiles + 37
  bits      (old_w + new_w) % 3 == 0 -> min(old_w, new_w) - 1 (the destination of adac_repack is wider than needed)
  position  (old_w + 2 new_w) % 3    -> bottom (new min = old min), top (the range ends on the frame's last field value),
                                        middle (a third of the way up, at an ODD offset: bottom and top move the range
                                        by a multiple of 2^bits, which the low new_w bits of a field do not show)
  frame     (old_w + new_w // 3) % 3 -> an arbitrary base (non-negative for the signed types); the frame that ends on the
                                        type's all-ones pattern (its unsigned maximum, -1 for a signed type); an
                                        all-negative frame at an arbitrary base (signed) or the frame at 0 (unsigned)
(old_w + new_w) and (old_w + 2 new_w) = (old_w - new_w) are independent mod 3, and 4 is prime to 3, so size, bits and
position meet in every combination the plane is large enough for.  A frame that spans the sign change is never packed
under either rule: such segments are the old_w = tb rows of a signed type.

The 8-byte plane and the register walk's stages: repack_run_w's stage is ((8 * 16384) / new_w) & ~127 rows, so the
longest segment of an 8-byte type (two tiles + 37 = 4133 rows) takes a second stage only at new_w = 32, which the size
rotation gives to old_w = 3 mod 4 alone.  For those types the generator appends, after the plane, one EXTRA segment
old_w -> 32 of two tiles + 37 rows for every other old_w in 4..32 (Case.extra marks them)."""
import collections

import numpy as np

ALL = [np.uint64, np.int64, np.uint32, np.int32, np.uint16, np.int16, np.uint8, np.int8]
TILE_BYTES, WORKGROUP = 16384, 256           # kTileBytes, kWorkgroup (csrc/adac_internal.h:13-14)
SIZES = ("3", "129", "tile", "2 tiles + 37")
POSITIONS = ("bottom", "top", "middle")
FRAMES = ("arbitrary", "ends on all-ones", "all-negative or zero")
U64 = 0xFFFFFFFFFFFFFFFF
# the widths of the NULL variant (both emissions, the byte and dword edges); the 1-byte types keep every width: their
# nine pairs of {1, 7, 8} could not start a validity window at every phase of a mask word
NULL_WIDTHS = (1, 7, 8, 9, 16, 17, 31, 32, 33, 63)
# new_w kept if the 8-byte plane has to be thinned (THIN_8_BYTE_PLANE); every old_w stays
THIN_NEW_W = tuple(range(1, 10)) + (13, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40, 48, 63, 64)
THIN_8_BYTE_PLANE = False                    # the full 4096-pair plane costs ~1 s of host work per call: not thinned


def tile_values(itemsize):
    return TILE_BYTES // itemsize


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' own predicates
def default_tiles_per_wg(itemsize):
    """ensure_scan_groups (csrc/adac_capi.cpp:1002-1006): the tiles a scan group gets at scan_tiles_per_wg = 0."""
    per = {8: 12, 4: 6, 2: 8, 1: 4}[itemsize]
    return min(per, 65536 // tile_values(itemsize))


def scan_groups(itemsize, count, tiles_per_wg=0):
    """[(first row, rows)] of a segment's scan groups (csrc/adac_capi.cpp:1007-1022): its tiles dealt evenly."""
    tile = tile_values(itemsize)
    per = tiles_per_wg if tiles_per_wg >= 1 else {8: 12, 4: 6, 2: 8, 1: 4}[itemsize]
    per = min(per, 65536 // tile)
    ntiles = (count + tile - 1) // tile
    if ntiles == 0:
        return []
    ngroups = (ntiles + per - 1) // per
    rows = (ntiles + ngroups - 1) // ngroups * tile
    return [(first, min(rows, count - first)) for first in range(0, count, rows)]


def register_walk_ok(old_w, count, validity, templated):
    """The part both kernels share (adac_kernels.hip:1754 and :1866): templated_scan on, no validity mask, a source
    width the walk is instantiated at, the segment below 2^31 bits."""
    return bool(templated) and not validity and 4 <= old_w <= 32 and count * old_w < (1 << 31)


def analyze_form(itemsize, old_w, count, validity=False, templated=True):
    """k_analyze_packed_g (adac_kernels.hip:1866): "register" (analyze_run_w) or "staged" (stage_packed + decode_run)."""
    return "register" if register_walk_ok(old_w, count, validity, templated) else "staged"


def repack_form(itemsize, old_w, new_w, count, validity=False, templated=True):
    """k_repack_g (adac_kernels.hip:1754, :1801): "register" (repack_run_w; also needs new_w <= 32), else the staged
    form with the 32-bit emission (chunk_string32 / image_or32, new_w <= 32) or the 64-bit one (concat_fields /
    image_or)."""
    if register_walk_ok(old_w, count, validity, templated) and new_w <= 32:
        return "register"
    return "staged32" if new_w <= 32 else "staged64"


def analyze_stage_rows(itemsize, old_w, form):
    """Rows per stage of k_analyze_packed_g: the register walk takes a whole group in one run (None: no stages,
    :1869); the staged form takes stage_tiles<U>(old_w, old_w) whole tiles (:1613-1620, :1888)."""
    if form == "register":
        return None
    tile = tile_values(itemsize)
    return max(1, (8 * TILE_BYTES) // (tile * old_w)) * tile


def repack_stage_rows(itemsize, old_w, new_w, form):
    """Rows per stage of k_repack_g: the output bits of a register stage fit the 16 KiB image (:1759); a staged stage
    is whole decode rounds whose packed bits fit 8 KiB on both sides, at least one round (:1788-1789)."""
    if form == "register":
        return ((8 * TILE_BYTES) // new_w) & ~127
    per_round = WORKGROUP * (16 // itemsize)
    rows = ((8 * (TILE_BYTES // 2)) // max(old_w, new_w)) // per_round * per_round
    return max(rows, per_round)


def stages_of(n, stage_rows):
    """(stages a group of n rows takes, is the last one partial)."""
    if stage_rows is None:
        return 1, False
    return (n + stage_rows - 1) // stage_rows, n % stage_rows != 0


Path = collections.namedtuple("Path", "analyze repack analyze_stages repack_stages analyze_partial repack_partial groups")


def path_of(itemsize, old_w, new_w, count, validity=False, templated=True, tiles_per_wg=0):
    """What one segment takes.  The stage counts are those of its LONGEST scan group (the first), the partial flags those
    of its last group."""
    an = analyze_form(itemsize, old_w, count, validity, templated)
    rp = repack_form(itemsize, old_w, new_w, count, validity, templated)
    groups = scan_groups(itemsize, count, tiles_per_wg)
    a_rows, r_rows = analyze_stage_rows(itemsize, old_w, an), repack_stage_rows(itemsize, old_w, new_w, rp)
    a_first, r_first = stages_of(groups[0][1], a_rows), stages_of(groups[0][1], r_rows)
    a_last, r_last = stages_of(groups[-1][1], a_rows), stages_of(groups[-1][1], r_rows)
    return Path(an, rp, a_first[0], r_first[0], a_last[1], r_last[1], len(groups))


# ---------------------------------------------------------------------------------------------------------------------
# the plane
Case = collections.namedtuple(
    "Case", "dtype counts old_w new_w bits size position frame extra base wide narrow dst_min val_offs validity valid")


def pair_size(old_w, new_w):
    return (old_w + new_w) % 4


def pair_bits(old_w, new_w):
    return min(old_w, new_w) - ((old_w + new_w) % 3 == 0)


def pair_position(old_w, new_w):
    return (old_w + 2 * new_w) % 3


def pair_frame(old_w, new_w):
    return (old_w + new_w // 3) % 3


def size_rows(itemsize, size):
    tile = tile_values(itemsize)
    return (3, 129, tile, 2 * tile + 37)[size]


def frame_base(rng, dtype, old_w, frame):
    """The old frame [base, base + 2^old_w) as T's bit patterns: it never wraps 2^tb, and for a signed type never spans
    the sign change unless old_w = tb."""
    tb = 8 * dtype.itemsize
    signed = dtype.kind == "i"
    if old_w == tb:
        return 0
    top = (1 << tb) - (1 << old_w)                       # the frame that ends on the all-ones pattern
    if frame == 1:
        return top
    if signed:
        half = 1 << (tb - 1)
        lo, hi = (0, half - (1 << old_w)) if frame == 0 else (half, top)
    else:
        lo, hi = (0, top) if frame == 0 else (0, 0)
    return lo + int(rng.integers(0, hi - lo + 1, dtype=np.uint64))


def pinned(rng, dtype, n, bits, low):
    """n values whose bit patterns lie in [low, low + 2^bits), both ends present (as make_values pins them)."""
    udt = np.dtype("u%d" % dtype.itemsize)
    span = rng.integers(0, 1 << bits, size=n, dtype=np.uint64) if bits else np.zeros(n, np.uint64)
    i0, i1 = rng.choice(n, size=2, replace=False)
    span[i0], span[i1] = 0, (1 << bits) - 1
    return ((span + np.uint64(low)) & np.uint64((1 << (8 * dtype.itemsize)) - 1)).astype(udt).view(dtype)


def plane_pairs(dtype, null_variant=False):
    """[(old_w, new_w, extra)] of one type's column, in segment order."""
    dtype = np.dtype(dtype)
    tb = 8 * dtype.itemsize
    if null_variant:
        keep = set(range(1, tb + 1)) if tb == 8 else {w for w in NULL_WIDTHS + (tb,) if w <= tb}
        return [(o, n, False) for o in sorted(keep) for n in sorted(keep)]
    new_ws = [n for n in range(1, tb + 1) if not (THIN_8_BYTE_PLANE and tb == 64) or n in THIN_NEW_W]
    pairs = [(o, n, False) for o in range(1, tb + 1) for n in new_ws]
    if tb == 64:                                         # see the module's note on the register walk's stages
        pairs += [(o, 32, True) for o in range(4, 33) if pair_size(o, 32) != 3]
    return pairs


def dst_min_of(low, bits, new_w, tb):
    """The min of the destination descriptor adac_repack is handed: the narrow values' minimum — except where that is
    the all-ones pattern of an 8-byte type, which a descriptor cannot hold (it reads as "no min"): the frame then starts
    2^new_w - 1 lower (the destination is wider than the constant segment needs anyway).  Unpacked: no min."""
    if new_w == tb:
        return U64
    if low == U64:
        return U64 - ((1 << new_w) - 1)
    return low


def make_case(dtype, null_variant=False, seed=0, pairs=None, rows_each=None):
    """The plane of one type (or its NULL variant); with `pairs` and `rows_each`, a column of those (old_w, new_w, extra)
    at that one size instead."""
    dtype = np.dtype(dtype)
    tb = 8 * dtype.itemsize
    rng = np.random.default_rng(7700 + 16 * seed + 2 * tb + (dtype.kind == "i") + 1000 * null_variant)
    pairs = plane_pairs(dtype, null_variant) if pairs is None else pairs
    counts, bits_l, sizes, positions, frames, bases, wide, narrow, dst_min = [], [], [], [], [], [], [], [], []
    for o, n, extra in pairs:
        size = 3 if extra else pair_size(o, n)
        rows = size_rows(dtype.itemsize, size) if rows_each is None else rows_each
        bits, pos, frame = pair_bits(o, n), pair_position(o, n), pair_frame(o, n)
        base = frame_base(rng, dtype, o, frame)
        room = (1 << o) - (1 << bits)
        low = base + (0, room, min(room, room // 3 | 1))[pos]
        counts.append(rows)
        bits_l.append(bits)
        sizes.append(size)
        positions.append(pos)
        frames.append(frame)
        bases.append(base)
        wide.append(pinned(rng, dtype, rows, o, base))
        narrow.append(pinned(rng, dtype, rows, bits, low))
        dst_min.append(dst_min_of(low, bits, n, tb))
    counts = np.array(counts, dtype=np.uint32)
    val_offs = validity = valid = None
    if null_variant:
        val_offs, valid = null_masks(rng, counts)
        validity = pack_bits(valid)
        for s, v in enumerate(narrow):                   # NULL slots of the source: arbitrary old_w-bit fields
            ok = valid[int(val_offs[s]):int(val_offs[s]) + len(v)]
            junk = pinned(rng, dtype, len(v), pairs[s][0], bases[s])
            v[~ok] = junk[~ok]
    return Case(dtype, counts, [p[0] for p in pairs], [p[1] for p in pairs], bits_l, sizes, positions, frames,
                [p[2] for p in pairs], bases, wide, narrow, dst_min, val_offs, validity, valid)


NULL_KINDS = ("dense", "all NULL", "all valid", "sparse", "runs")


def null_masks(rng, counts):
    """Value offsets with a non-zero gap before every segment, chosen so that segment s starts at bit (37 s + 1) % 64
    of a mask word, and the validity bits of the whole span: segment s is of NULL_KINDS[s % 5]."""
    offs, run = [], 0
    for s, c in enumerate(counts):
        gap = ((37 * s + 1) - run) % 64
        run += gap if gap else 64
        offs.append(run)
        run += int(c)
    valid = rng.random(run) > 0.5                        # the gaps: bits that belong to no segment
    for s, (o, c) in enumerate(zip(offs, counts)):
        c = int(c)
        kind = NULL_KINDS[s % 5]
        if kind == "dense":
            bits = rng.random(c) > 0.3
        elif kind == "all NULL":
            bits = np.zeros(c, bool)
        elif kind == "all valid":
            bits = np.ones(c, bool)
        elif kind == "sparse":
            bits = rng.random(c) > 0.95
        else:
            bits = (np.arange(c) // int(rng.integers(1, 71))) % 2 == 0
        valid[o:o + c] = bits
    return np.array(offs, dtype=np.uint64), valid


def pack_bits(valid):
    vm = np.packbits(valid, bitorder="little")
    return np.concatenate([vm, np.zeros((-len(vm)) % 8 + 8, np.uint8)]).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# the two small columns
def cross_rule_column(dtype, seed=0):
    """For a signed type: (counts, segments) that change their min/max representation between the rules.  All-negative
    segments at a few widths — packed under both rules, min sign-extended under RULE_APPEND and zero-extended under
    RULE_RECOMPACT — and segments in [-k, k], which neither rule packs.  Sizes: one that the register walk takes in one
    chunk round, a tile, and two tiles + 37."""
    dtype = np.dtype(dtype)
    assert dtype.kind == "i"
    tb = 8 * dtype.itemsize
    rng = np.random.default_rng(8800 + tb + seed)
    tile = tile_values(dtype.itemsize)
    segs = []
    for i, w in enumerate(sorted({1, 3, 4, 7, 9, 13, 17, 31, 33, tb - 1} & set(range(1, tb)))):
        n = (129, tile, 2 * tile + 37)[i % 3]
        half, top = 1 << (tb - 1), (1 << tb) - (1 << w)
        base = top if i % 2 else half + int(rng.integers(0, top - half + 1, dtype=np.uint64))
        segs.append(pinned(rng, dtype, n, w, base))      # all-negative; every other one ends on -1
    for i, k in enumerate((1, 5, (1 << (tb - 1)) - 1)):
        n = (tile, 129, 2 * tile + 37)[i]
        v = rng.integers(-k, k + 1, size=n, dtype=np.int64).astype(dtype)
        v[:2] = (-k, k)
        segs.append(v)
    return np.array([len(v) for v in segs], dtype=np.uint32), segs


# (old_w, new_w) of the several-groups column: the register walk at three source widths, the staged form below width
# 4 and (8-byte types) above 32 bits.  Widths the type does not have are clamped to tb (13 -> 17 is 13 -> 16 for the
# 2-byte types) and pairs whose old_w it does not have are dropped.
GROUP_PAIRS = ((5, 3), (13, 17), (32, 32), (3, 2), (40, 33))
GROUP_TILES_PER_WG = 2


def group_pairs(dtype):
    tb = 8 * np.dtype(dtype).itemsize
    return [(o, min(n, tb)) for o, n in GROUP_PAIRS if o <= tb]


def group_rows(dtype):
    return 5 * tile_values(np.dtype(dtype).itemsize) + 37


def make_group_case(dtype):
    """One segment of 5 tiles + 37 rows per pair of group_pairs: three scan groups at GROUP_TILES_PER_WG, the last partial."""
    return make_case(dtype, seed=5, pairs=[(o, n, False) for o, n in group_pairs(dtype)], rows_each=group_rows(dtype))
