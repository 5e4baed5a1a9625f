"""The persistent kernels at workgroup counts other than the whole device's (tuning knob "num_cus").

k_encode_1p launches min(segments, CUs) workgroups that take segments from a ticket counter; k_group_sum_rw / k_group_sum
launch up to 7 x CUs.  On a whole MI355X that count is 256, so with up to 256 segments no encode workgroup ever hands
its state (LDS pool, prefetched rounds, next_loaded / next_ticket, the pending parked or big-image segment) from one
segment to the next, and the grouped scan's workgroups loop once or twice.  Here:

  A. num_cus = 1 and single_pass_encode = 2: ONE workgroup takes segments 0, 1, 2, ... in order, so every segment's
     predecessor is known.  The column is an Eulerian walk over the complete digraph of segment kinds (one kind per
     flow of adac_encode_1p.inl, see flow_of below): every ordered pair kind a -> kind b, self-pairs included, exactly
     once; rotations of the walk end on every kind in turn.  Every type, both rules, padded, NULL masks, the
     encode_big_image / encode_publish_ahead knobs, both placements; then 2 and 3 workgroups on the same walk, and 32 / 64 /
     128 (the partition sizes) on a few hundred segments.  Under ordered placement descriptors and arena are byte-identical
     to the default grid's.  The stamps test proves the knob reaches the kernel.
  B. the fuzz generator of test_gpu_fuzz.py (1 - 8 segments: never a hand-over at the default grid) on 1 and 2 workgroups.
  C. the grouped scan on 7 .. 896 workgroups that loop over tens to hundreds of scan groups, with ngroups around
     kGroupPrivateBins, both kernel forms, group_sum_wide 0 and 1.
  D. the two gather forms adac_unpack_selected does not select by default (gather_compact 0 and 1).

Encode is compared word for word with the CPU oracle, the scans with numpy over the raw columns: no tolerances.
Every knob is process-global: each set_tuning is undone in a `finally`, and the last test checks the defaults."""
import ctypes
import functools
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_parity as parity
from test_gpu_fuzz import random_case
from test_gpu_group_sum import encode_column, reference_groups, run_case
from test_gpu_group_sum_rw import both_ways, every_width_column, mixed_walk_column
from test_gpu_parity import check_placement, make_values, mixed_flow_column, run_encode_decode
from test_gpu_select import many_groups_column, pack_mask, ragged_gather_column

gpu = pytest.mark.gpu

ALL = [np.uint64, np.int64, np.uint32, np.int32, np.uint16, np.int16, np.uint8, np.int8]
DEFAULTS = {"num_cus": 0, "single_pass_encode": 1, "encode_placement": 0, "encode_big_image": 1, "encode_publish_ahead": 1,
            "gather_compact": 3, "group_sum_wide": 0, "group_sum_rw": 1, "encode_stamps": 0}


class knobs:
    """with knobs(adac, num_cus=1, ...): the knobs set on entry, their defaults restored on exit (also on a failure)."""

    def __init__(self, adac, **values):
        self.adac, self.values = adac, values

    def __enter__(self):
        try:
            for k, v in self.values.items():
                assert k in DEFAULTS, k
                self.adac.set_tuning(k, v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for k in self.values:
            self.adac.set_tuning(k, DEFAULTS[k])
        return False


@functools.lru_cache(maxsize=None)
def device_cus():
    """torch's multi_processor_count of device 0, asked for in a child process: the codec library has brought its own
    HIP runtime into this one, and torch's cannot initialise next to it ("No HIP GPUs are available")."""
    code = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True, timeout=300).stdout
    n = int(out.strip().splitlines()[-1])
    assert n > 0
    return n


def grids(wanted):
    """The sweep values the device can hold resident: the encode's look-back spins, so num_cus never exceeds the CU count."""
    have = device_cus()
    return [g for g in wanted if g <= have]


# ------------------------------------------------------------------------------------------------------------------
# A. the segment kinds: one per flow of k_encode_1p (adac_encode_1p.inl, "phase 4" and section 4a)
# ------------------------------------------------------------------------------------------------------------------
ENC_THREADS, ENC_ROUNDS, ENC_PREFETCH, ENC_IMAGE_WORDS = 1024, 16, 6, 48 * 1024 // 8
POOL_WORDS = (ENC_PREFETCH * ENC_THREADS * 16 + (ENC_IMAGE_WORDS + 4) * 8) // 8 - 4
ONE_PASS_BYTES = 16 * 1024 * 16       # kEncodeOnePassBytes: (align + rows) of a segment the single pass takes


def flow_of(itemsize, w, n, align, has_next, validity=False, first_come=False, big_image=True):
    """The kernel's own predicates: which flow segment (n rows at width w, `align` rows after a 16-byte boundary) takes."""
    K, tb = 16 // itemsize, 8 * itemsize
    if n == 0:
        return "empty"
    whole_dwords = not validity and (K * w) % 32 == 0 and (align * w) % 32 == 0 and (w <= 32 or w == tb)
    parked = whole_dwords and K * w <= 64
    seg_words = (n * w + 63) >> 6
    bigimg = ((not whole_dwords or (parked and K * w == 32)) and not validity and w <= 32 and seg_words + 2 <= POOL_WORDS
              and ENC_ROUNDS * ENC_THREADS * K * w + 128 <= POOL_WORDS * 64 and has_next and not first_come and big_image)
    if bigimg:
        return "big image"
    if parked:
        return "parked"
    return "wide" if whole_dwords else "staged"


def kind_table(dtype):
    """{kind: (width, placement class)} for one type; placement 'a' = chunk-aligned, 'm' = misaligned, '*' = rotates."""
    itemsize = np.dtype(dtype).itemsize
    K, tb = 16 // itemsize, 8 * itemsize
    fits = [w for w in range(1, min(tb, 33)) if (K * w) % 32 and ENC_ROUNDS * ENC_THREADS * K * w + 128 <= POOL_WORDS * 64]
    big = max(fits)                                           # the widest image a full segment still fits the pool with
    staged = min(w for w in range(big + 1, tb) if (K * w) % 32 and not (w <= 32 and w in fits))
    kinds = {"empty": (0, "*"), "single": (1, "*"), "park2": (64 // K, "a"), "one aligned": (32 // K, "a"),
             "one misaligned": (32 // K, "m"), "big": (big, "*"), "staged": (staged, "*"), "unpacked": (tb, "*"),
             "constant": (1, "*")}
    wide = [w for w in range(1, min(tb, 33)) if (K * w) % 32 == 0 and K * w > 64]
    if wide:                                                  # (the 8-byte types have none below 64 bits)
        kinds["wide"] = (wide[0], "a")
    return kinds


def euler_walk(k, seed=2718):
    """A closed walk over the complete digraph on k nodes with self-loops that uses each of its k * k edges once
    (Hierholzer, edges taken in a seeded random order): k * k + 1 nodes, the first repeated at the end."""
    rng = np.random.default_rng(seed)
    out = [list(rng.permutation(k)) for _ in range(k)]
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(int(out[v].pop()))
        else:
            walk.append(stack.pop())
    return walk[::-1]


def walk_kinds(dtype, rotation=0):
    """The kind sequence of the walk column; rotation r starts the closed walk at its r-th node (and ends on that node)."""
    names = list(kind_table(dtype))
    seq = euler_walk(len(names))
    m = len(seq) - 1
    rot = seq[rotation:m] + seq[:rotation + 1]
    return [names[i] for i in rot]


def rotation_ending_on(dtype, kind):
    names = list(kind_table(dtype))
    return euler_walk(len(names)).index(names.index(kind))


def walk_column(dtype, kinds_seq, seed=0, limit_rows=None):
    """Segments for a kind sequence: (counts, seg_vals, val_offs, widths expected under the append rule, aligns).
    Sizes rotate per kind over a small count, a stage (or round) boundary - 1, + 0, + 1 and a full block; placements
    over chunk-aligned and misaligned value offsets unless the kind fixes one."""
    dtype = np.dtype(dtype)
    itemsize = dtype.itemsize
    K, tb = 16 // itemsize, 8 * itemsize
    table = kind_table(dtype)
    full = 262136 // itemsize
    round_rows = ENC_THREADS * K
    rng = np.random.default_rng(4000 + 16 * seed + tb + (dtype.kind == "i"))
    seen = {k: 0 for k in table}
    counts, segs, offs, widths, aligns, run = [], [], [], [], [], 0
    for pos, kind in enumerate(kinds_seq):
        w, pclass = table[kind]
        i = seen[kind]
        seen[kind] += 1
        rps = max(1, ENC_IMAGE_WORDS * 64 // (round_rows * max(w, 1)))
        sb = rps * round_rows if rps * round_rows + 1 < full else round_rows
        n = {"empty": 0, "single": 1}.get(kind, [37 + pos % 23, sb - 1, full, sb + 1, sb][i % 5])
        if limit_rows:
            n = min(n, limit_rows)
        align = {"a": 0, "m": (1, K - 1)[i % 2], "*": (0, 1, K - 1, K // 2)[i % 4]}[pclass]
        if (align + n) * itemsize > ONE_PASS_BYTES:    # or the layout would leave the single pass for the three kernels
            align = 1 if pclass == "m" else 0
        run += (0, 2 * K, 0, 5)[pos % 4]                # gaps between the segments, some none
        run += (align - run) % K
        if kind == "constant":
            v = np.full(n, int(rng.integers(1, 100)), dtype=dtype)
        elif kind == "unpacked":                        # over the whole range of T (mixed sign for the signed types)
            v = make_values(rng, dtype, n, tb, base=0)
        else:                                           # a frame of reference on either side of zero, never across it
            top = 1 << w
            base = (3 if top + 3 <= 1 << (tb - 1) else 0) if i % 2 == 0 else (1 << tb) - top - (2 if w < tb - 1 else 0)
            v = make_values(rng, dtype, n, w, base=base) if n else np.zeros(0, dtype)
        counts.append(n)
        segs.append(v)
        offs.append(run)
        widths.append(w)
        aligns.append(align)
        run += n
    return np.array(counts, dtype=np.uint32), segs, np.array(offs, dtype=np.uint64), widths, aligns


def null_mask(rng, counts, offs, all_null_segment):
    """Validity over the column's value span: ~25 % NULL rows, and one segment without a single valid row."""
    span = int(offs[-1]) + int(counts[-1])
    valid = rng.random(span) > 0.25
    o, c = int(offs[all_null_segment]), int(counts[all_null_segment])
    valid[o:o + c] = False
    return pack_mask(valid, span)


def arena(lay, d_words):
    return d_words.download(np.uint64, lay.max_arena_words)


def encode_first_come(adac, oracle, ctx, dtype, counts, segs, offs, rule=0, padded=False, validity=None):
    """run_encode_decode under first-come placement: per segment against the oracle at the offset the kernel chose,
    plus check_placement (what test_single_pass_encode_mixes_its_flows asks of that placement)."""
    adac.set_tuning("encode_placement", 1)
    parity.FIRST_COME = True
    try:
        lay, _, _, descs, _ = run_encode_decode(adac, oracle, ctx, dtype, counts, segs, rule, padded, validity, offs)
    finally:
        parity.FIRST_COME = False
        adac.set_tuning("encode_placement", 0)
    check_placement(adac, descs, lay.max_arena_words)
    return descs


@pytest.mark.parametrize("dtype", ALL)
def test_walk_visits_every_ordered_pair_of_kinds(adac, oracle, dtype):
    """No GPU: the generated sequence holds every ordered pair (kind a -> kind b) once, every rotation ends on the kind
    asked for, every kind gets every size and the placements it may take, the oracle gives every segment the width its
    kind stands for, the kernel's predicates put every kind into the flow it is named after, and every segment fits the
    single-pass kernel (else adac_encode would silently take the three kernels)."""
    dtype = np.dtype(dtype)
    table = kind_table(dtype)
    names = list(table)
    K = 16 // dtype.itemsize
    assert len(names) == (9 if dtype.itemsize == 8 else 10)
    for kind in names:
        seq = walk_kinds(dtype, rotation_ending_on(dtype, kind))
        assert seq[-1] == kind and len(seq) == len(names) ** 2 + 1
        pairs = set(zip(seq[:-1], seq[1:]))
        assert pairs == {(a, b) for a in names for b in names}, kind
    seq = walk_kinds(dtype)
    counts, segs, offs, widths, aligns = walk_column(dtype, seq, limit_rows=5000)   # (the widths: on short segments)
    for s, (kind, v) in enumerate(zip(seq, segs)):
        if len(v):
            mn, mx = oracle.analyze_flat(v, 0)
            w = oracle.width_from_succinct(mn, mx, False)
            assert min(w, 8 * dtype.itemsize) == table[kind][0], (kind, s, w)
    counts, segs, offs, widths, aligns = walk_column(dtype, seq)
    assert all(int(o) % K == a for o, a in zip(offs, aligns))
    assert all(int(offs[i]) + int(counts[i]) <= int(offs[i + 1]) for i in range(len(seq) - 1))
    assert all((a + int(c)) * dtype.itemsize <= ONE_PASS_BYTES for a, c in zip(aligns, counts))
    full = 262136 // dtype.itemsize
    for kind in names:
        mine = [i for i, k in enumerate(seq) if k == kind]
        if kind not in ("empty", "single"):
            sizes = {int(counts[i]) for i in mine}
            assert full in sizes and min(sizes) < 64 and len(sizes) >= 5, (kind, sizes)
        if table[kind][1] == "*" and K > 2:
            assert {aligns[i] for i in mine if counts[i] < full} >= {0, 1, K - 1}, kind
    expect = {"empty": {"empty"}, "single": {"big image"}, "park2": {"parked"}, "one aligned": {"big image"},
              "one misaligned": {"big image"}, "big": {"big image"}, "staged": {"staged"}, "wide": {"wide"},
              "constant": {"big image"}}
    for s, kind in enumerate(seq[:-1]):
        f = flow_of(dtype.itemsize, widths[s], int(counts[s]), aligns[s], True)
        if kind == "unpacked":     # the rows are the words: straight from the registers where the placement allows
            assert f == ("wide" if (aligns[s] * widths[s]) % 32 == 0 else "staged")
        else:
            assert f in expect[kind], (kind, s, f)
        if kind == "one aligned":  # ... and parks when it is the last segment, the big image is off or first come places
            assert flow_of(dtype.itemsize, widths[s], int(counts[s]), aligns[s], False) == "parked"
        if kind == "one misaligned":
            assert flow_of(dtype.itemsize, widths[s], int(counts[s]), aligns[s], True, first_come=True) == "staged"
    # a full staged segment takes several stages
    w = table["staged"][0]
    assert ENC_ROUNDS // max(1, ENC_IMAGE_WORDS * 64 // (ENC_THREADS * K * w)) >= 3


def ordered(adac, oracle, ctx, dtype, col, rule=0, padded=False, validity=None):
    counts, segs, offs = col[:3]
    lay, d_words, _, descs, _ = run_encode_decode(adac, oracle, ctx, dtype, counts, segs, rule, padded, validity, offs)
    return descs.tobytes(), arena(lay, d_words), descs


_first = {}


@gpu
def test_a_dozen_segments_on_one_workgroup(adac, oracle, gpu_ctx):
    """The smallest case, first: uint64, twelve short segments of the walk, one workgroup."""
    dtype = np.dtype(np.uint64)
    col = walk_column(dtype, walk_kinds(dtype)[:12], limit_rows=3000)
    _first["default"] = ordered(adac, oracle, gpu_ctx, dtype, col)[:2]      # before any knob was touched
    with knobs(adac, single_pass_encode=2):
        ref = ordered(adac, oracle, gpu_ctx, dtype, col)
        with knobs(adac, num_cus=1):
            one = ordered(adac, oracle, gpu_ctx, dtype, col)
            encode_first_come(adac, oracle, gpu_ctx, dtype, *col[:3])
    assert one[0] == ref[0] == _first["default"][0] and np.array_equal(one[1], ref[1])
    assert np.array_equal(ref[1], _first["default"][1])


def stamp_places(adac, nseg):
    """The CU (XCC, SE, SH, CU of the hardware id in stamp slot 7) every segment of the last stamped encode ran on."""
    buf = np.zeros((nseg, 8), dtype=np.uint64)
    rc = adac.lib().adac_debug_encode_stamps(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(buf.nbytes))
    assert rc == 0
    hw = buf[:, 7]
    return (((hw >> np.uint64(32)) & np.uint64(0xf)) << np.uint64(16)) | ((hw >> np.uint64(8)) & np.uint64(0xff))


def stamped_places(adac, oracle, ctx, num_cus):
    dtype = np.dtype(np.uint64)
    rng = np.random.default_rng(17)
    counts = np.full(300, 20000, dtype=np.uint32)
    segs = [make_values(rng, dtype, 20000, 13 + s % 3) for s in range(300)]
    with knobs(adac, single_pass_encode=2, encode_stamps=1, num_cus=num_cus):
        run_encode_decode(adac, oracle, ctx, dtype, counts, segs)
        return set(stamp_places(adac, 300).tolist())


@gpu
def test_num_cus_reaches_the_encode_kernel(adac, oracle, gpu_ctx):
    """Without this the rest proves nothing: with one workgroup every segment's stamp record names the same CU, with
    two at most two CUs, and the default grid spreads 300 segments over many."""
    assert len(stamped_places(adac, oracle, gpu_ctx, 1)) == 1
    assert len(stamped_places(adac, oracle, gpu_ctx, 2)) <= 2
    assert len(stamped_places(adac, oracle, gpu_ctx, 0)) > 2


@gpu
@pytest.mark.parametrize("dtype", ALL)
def test_every_hand_over_in_a_fixed_order(adac, oracle, gpu_ctx, dtype):
    """One workgroup walks every ordered pair of kinds: both rules, padded on and off, with and without NULLs (one
    segment all NULL), the big image and publish-ahead each on and off, first-come placement; then two and three
    workgroups alternate through the same walk.  Ordered placement: the bytes of the default grid."""
    dtype = np.dtype(dtype)
    seq = walk_kinds(dtype)
    col = walk_column(dtype, seq)
    counts, segs, offs = col[:3]
    rng = np.random.default_rng(5 + dtype.itemsize)
    all_null = next(s for s, k in enumerate(seq) if k == "park2" and counts[s] > 64)
    vm = null_mask(rng, counts, offs, all_null)
    with knobs(adac, single_pass_encode=2):
        ref = {}
        for rule in (adac.RULE_APPEND, adac.RULE_RECOMPACT):
            for padded in (False, True):
                for mask in (None, vm):
                    ref[rule, padded, mask is None] = ordered(adac, oracle, gpu_ctx, dtype, col, rule, padded, mask)
        d1 = ref[adac.RULE_APPEND, False, True][2]
        assert [min(w, 8 * dtype.itemsize) for w in col[3]] == [int(w) if c else 0 for w, c in zip(d1["width"], counts)]
        assert int(ref[adac.RULE_APPEND, False, False][2]["min"][all_null]) == parity.U64
        for cus in grids([1, 2, 3]):
            with knobs(adac, num_cus=cus):
                for (rule, padded, nomask), (db, words, _) in ref.items():
                    got = ordered(adac, oracle, gpu_ctx, dtype, col, rule, padded, None if nomask else vm)
                    assert got[0] == db and np.array_equal(got[1], words), (cus, rule, padded, nomask)
                for big, ahead in ((0, 1), (1, 0), (0, 0)):
                    with knobs(adac, encode_big_image=big, encode_publish_ahead=ahead):
                        got = ordered(adac, oracle, gpu_ctx, dtype, col)
                        assert got[0] == d1.tobytes() and np.array_equal(got[1], ref[adac.RULE_APPEND, False, True][1]), (cus, big, ahead)
                        if cus == 1:
                            got = ordered(adac, oracle, gpu_ctx, dtype, col, adac.RULE_RECOMPACT, True, vm)
                            masked = ref[adac.RULE_RECOMPACT, True, False]
                            assert got[0] == masked[0] and np.array_equal(got[1], masked[1]), (big, ahead)
                df = encode_first_come(adac, oracle, gpu_ctx, dtype, counts, segs, offs)
                for f in ("count", "width", "flags", "min", "val_off"):
                    assert np.array_equal(df[f], d1[f]), (cus, f)
                encode_first_come(adac, oracle, gpu_ctx, dtype, counts, segs, offs, adac.RULE_RECOMPACT, True, vm)


@gpu
@pytest.mark.parametrize("dtype", ALL)
def test_every_kind_as_a_workgroups_last_segment(adac, oracle, gpu_ctx, dtype):
    """Rotations of the walk that end on each kind in turn: the column's last segment is the one workgroup's last."""
    dtype = np.dtype(dtype)
    with knobs(adac, single_pass_encode=2):
        for r, kind in enumerate(kind_table(dtype)):
            seq = walk_kinds(dtype, rotation_ending_on(dtype, kind))
            col = walk_column(dtype, seq, seed=1 + r, limit_rows=(None, 40000)[r % 2])
            ref = ordered(adac, oracle, gpu_ctx, dtype, col)
            with knobs(adac, num_cus=1):
                got = ordered(adac, oracle, gpu_ctx, dtype, col)
                assert got[0] == ref[0] and np.array_equal(got[1], ref[1]), kind
                encode_first_come(adac, oracle, gpu_ctx, dtype, *col[:3])


def doubled(counts, segs, offs):
    span = int(offs[-1]) + int(counts[-1])
    span += (-span) % 16
    return (np.concatenate([counts, counts]), segs + segs, np.concatenate([offs, offs + np.uint64(span)]))


@gpu
@pytest.mark.parametrize("dtype", ALL)
def test_partition_sized_grids_on_many_segments(adac, oracle, gpu_ctx, dtype):
    """32, 64 and 128 workgroups (the CU counts of a partitioned device) on the 700 random segments of
    test_single_pass_encode_mixes_its_flows, twice over: 11 to 44 segments per workgroup."""
    dtype = np.dtype(dtype)
    counts, segs, _, offs = mixed_flow_column(dtype, 700)
    col = doubled(counts, segs, offs)
    with knobs(adac, single_pass_encode=2):
        ref = ordered(adac, oracle, gpu_ctx, dtype, col)
        for cus in grids([32, 64, 128]):
            with knobs(adac, num_cus=cus):
                got = ordered(adac, oracle, gpu_ctx, dtype, col)
                assert got[0] == ref[0] and np.array_equal(got[1], ref[1]), cus
                df = encode_first_come(adac, oracle, gpu_ctx, dtype, *col)
                for f in ("count", "width", "flags", "min", "val_off"):
                    assert np.array_equal(df[f], ref[2][f]), (cus, f)


# ------------------------------------------------------------------------------------------------------------------
# B. the fuzz generator under small grids
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("seed", range(0, 120, 3))
def test_random_columns_on_one_and_two_workgroups(adac, oracle, gpu_ctx, seed):
    rng = np.random.default_rng(10_000 + seed)          # the columns, rules and masks of test_random_columns
    dtype, counts, segs, offs, span = random_case(rng, adac)
    rule = adac.RULE_APPEND if rng.random() < 0.6 else adac.RULE_RECOMPACT
    padded = bool(rng.random() < 0.3)
    vm = None
    if rng.random() < 0.4 and span:
        vm = pack_mask(rng.random(span) > rng.random() * 0.8, span)
    with knobs(adac, single_pass_encode=2):
        ref = ordered(adac, oracle, gpu_ctx, dtype, (counts, segs, offs), rule, padded, vm)
        for cus in grids([1, 2]):
            with knobs(adac, num_cus=cus):
                got = ordered(adac, oracle, gpu_ctx, dtype, (counts, segs, offs), rule, padded, vm)
                assert got[0] == ref[0] and np.array_equal(got[1], ref[1]), cus
                encode_first_come(adac, oracle, gpu_ctx, dtype, counts, segs, offs, rule, padded, vm)


# ------------------------------------------------------------------------------------------------------------------
# C. the grouped scan with few and with many rounds per workgroup
# ------------------------------------------------------------------------------------------------------------------
GROUP_GRIDS = [1, 2, 32, 64, 128]


def group_scan_sweep(adac, ctx, vals, keys, counts, ngroups, grid_sizes, voffs=None, koffs=None):
    """both_ways' three calls (register walk, staged kernel alone, register walk again: the hand-over word) at every
    grid size, in narrow and in 64-bit arithmetic, against numpy's GROUP BY over the raw columns.  The columns are
    encoded once; every scan call is followed by a second one, so both call parities see every configuration."""
    vlay, vwords = encode_column(adac, ctx, vals, counts, voffs)
    klay, kwords = encode_column(adac, ctx, keys, counts, koffs)
    d_sums, d_cnts = ctx.alloc((ngroups + 1) * 8), ctx.alloc((ngroups + 1) * 8)
    exp_s, exp_c = reference_groups(vals, keys, ngroups)
    poison = np.full(ngroups + 1, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    for wide in (0, 1):
        for cus in grid_sizes:
            for rw in (1, 0, 1):
                with knobs(adac, group_sum_wide=wide, num_cus=cus, group_sum_rw=rw):
                    for rep in range(2):
                        d_sums.upload(poison)
                        d_cnts.upload(poison)
                        vlay.scan_group_sum(vwords, klay, kwords, ngroups, d_sums, d_cnts)
                        assert d_cnts.download(np.uint64, ngroups + 1).tolist() == exp_c, (wide, cus, rw, rep)
                        assert d_sums.download(np.uint64, ngroups + 1).tolist() == exp_s, (wide, cus, rw, rep)
    return vlay.get_descs(), klay.get_descs()


@gpu
def test_group_scan_smallest_case_first(adac, gpu_ctx):
    """both_ways itself on one workgroup per kernel slot (7 workgroups), before the sweeps."""
    vals, keys, counts = mixed_walk_column(np.random.default_rng(5150))
    for wide in (0, 1):
        with knobs(adac, num_cus=1, group_sum_wide=wide):
            try:
                both_ways(adac, gpu_ctx, vals, keys, counts, 6)
                both_ways(adac, gpu_ctx, vals, keys, counts, 6)
            finally:
                adac.set_tuning("group_sum_rw", 1)


@gpu
@pytest.mark.parametrize("vdtype", [np.uint32, np.int32, np.uint64, np.uint16])
def test_group_scan_every_value_width_at_every_grid(adac, gpu_ctx, vdtype):
    """The every-value-width column of test_every_value_width_against_every_key_width at a few key widths, with
    ngroups 1, 7, 8, 9 and 256: 7 and 8 straddle kGroupPrivateBins (register walk | staged kernel)."""
    vdtype = np.dtype(vdtype)
    rng = np.random.default_rng(31 + vdtype.itemsize)
    widths, counts, vals = every_width_column(rng, vdtype)
    for wk, ngroups, kbase in ((1, 1, 0), (3, 7, 0), (3, 8, 2), (4, 8, 0), (5, 9, 0), (8, 7, 0), (9, 256, 0)):
        keys = (rng.integers(0, 2 ** wk, size=len(vals)) + kbase).astype(np.uint8 if wk < 8 else np.uint16)
        vd, kd = group_scan_sweep(adac, gpu_ctx, vals, keys, counts, ngroups, grids(GROUP_GRIDS))
        assert sorted(set(vd["width"].tolist())) == widths and set(kd["width"].tolist()) <= {wk, wk + 1}


@gpu
def test_group_scan_mixed_segments_at_every_grid(adac, gpu_ctx):
    """The column of test_segments_the_register_walk_leaves_to_the_staged_kernel: fall-backs are counted per workgroup."""
    vals, keys, counts = mixed_walk_column(np.random.default_rng(5150))
    for ngroups in (1, 6, 7, 8, 9, 256):
        vd, kd = group_scan_sweep(adac, gpu_ctx, vals, keys, counts, ngroups, grids(GROUP_GRIDS))
        assert vd["width"].tolist()[:5] == [2, 40, 13, 1, 24] and kd["width"].tolist()[2] == 10
    group_scan_sweep(adac, gpu_ctx, vals.view(np.uint64), keys, counts, 7, grids(GROUP_GRIDS))
    group_scan_sweep(adac, gpu_ctx, (vals & 0x7fffffff).astype(np.uint32), keys.astype(np.uint8), counts, 3, grids(GROUP_GRIDS))


@gpu
def test_group_scan_with_gaps_at_every_grid(adac, gpu_ctx):
    """run_case with gapped columns (test_group_sum_placements_and_wide_keys), each scan repeated on the same layouts."""
    counts = np.array([1000, 37, 5000, 2048, 1, 16385], dtype=np.uint32)
    cases = ((np.int32, np.uint8, 4, 21, 4), (np.uint64, np.uint64, 8, 47, 2 ** 40), (np.int64, np.int16, 200, 33, 200),
             (np.uint16, np.uint8, 7, 9, 9), (np.uint8, np.uint8, 1, 5, 3), (np.int32, np.uint16, 9, 30, 12),
             (np.uint32, np.uint16, 256, 17, 300))
    for wide in (0, 1):
        for cus in grids(GROUP_GRIDS):
            with knobs(adac, group_sum_wide=wide, num_cus=cus):
                rng = np.random.default_rng(99)
                for vdt, kdt, ngroups, vbits, key_top in cases:
                    vlay, vwords, klay, kwords = run_case(adac, gpu_ctx, rng, vdt, kdt, counts, ngroups, vbits, key_top, gaps=True)
                    d_s, d_c = gpu_ctx.alloc((ngroups + 1) * 8), gpu_ctx.alloc((ngroups + 1) * 8)
                    vlay.scan_group_sum(vwords, klay, kwords, ngroups, d_s, d_c)
                    first = d_s.download(np.uint64, ngroups + 1).tolist(), d_c.download(np.uint64, ngroups + 1).tolist()
                    vlay.scan_group_sum(vwords, klay, kwords, ngroups, d_s, d_c)
                    again = d_s.download(np.uint64, ngroups + 1).tolist(), d_c.download(np.uint64, ngroups + 1).tolist()
                    assert first == again and sum(first[1]) == int(counts.sum()), (wide, cus, ngroups)


@gpu
@pytest.mark.parametrize("vdtype,kdtype", [(np.uint32, np.uint8), (np.int64, np.uint16)])
def test_group_scan_hundreds_of_rounds_per_workgroup(adac, gpu_ctx, vdtype, kdtype):
    """1500 segments of one scan group each: with num_cus = 1 each of the seven workgroups loops over more than two
    hundred groups of changing segment, width and frame of reference, its private bins carried across all of them."""
    vdtype = np.dtype(vdtype)
    rng = np.random.default_rng(808 + vdtype.itemsize)
    tile = adac.tile_values(vdtype)
    counts = rng.integers(1, 2 * tile, size=1500).astype(np.uint32)
    counts[::97] = 0
    widths = rng.choice([1, 3, 4, 5, 9, 13, 16, 20, 24, 31], size=len(counts))
    vals = np.concatenate([make_values(rng, vdtype, int(c), int(w), base=5 + int(w)) for c, w in zip(counts, widths)])
    for ngroups, key_top in ((7, 7), (8, 10), (256, 300)):
        keys = rng.integers(0, key_top, size=len(vals)).astype(kdtype)
        keys[:int(counts[:700].sum())] %= 4                 # narrower key segments in the first half
        group_scan_sweep(adac, gpu_ctx, vals, keys, counts, ngroups, grids([1, 2, 32]))


# ------------------------------------------------------------------------------------------------------------------
# D. the two gather forms that are not selected by default
# ------------------------------------------------------------------------------------------------------------------
def check_gather_forms(adac, ctx, lay, d_words, dtype, counts, segs, offs, span, rng):
    total_rows = int(counts.sum())
    d_out = ctx.alloc(total_rows * dtype.itemsize + 64)
    d_ids = ctx.alloc(total_rows * 8 + 64)
    owned = np.zeros(span, dtype=bool)
    for v, o in zip(segs, offs):
        owned[o:o + len(v)] = True
    last = max(o + len(v) for v, o in zip(segs, offs)) - 1
    sels = {"empty": np.zeros(span, dtype=bool), "full": owned.copy(), "last row": np.zeros(span, dtype=bool),
            "clustered": np.zeros(span, dtype=bool), "scattered": owned & (rng.random(span) < 0.3)}
    sels["last row"][last] = True
    sels["clustered"][span // 2:span // 2 + span // 10] = True
    sels["clustered"] &= owned
    for name, sel in sels.items():
        d_bm = ctx.upload(pack_mask(sel, span)[:(span + 63) // 64])
        exp_vals = np.concatenate([v[sel[o:o + len(v)]] for v, o in zip(segs, offs)])
        exp_ids = np.concatenate([o + np.flatnonzero(sel[o:o + len(v)]) for v, o in zip(segs, offs)]).astype(np.uint64)
        for form in (3, 0, 1, 3):
            with knobs(adac, gather_compact=form):
                n = lay.unpack_selected(d_words, d_bm, d_out, d_ids)
                assert n == len(exp_vals), (name, form)
                assert np.array_equal(d_out.download(dtype, max(n, 1))[:n], exp_vals), (name, form)
                assert np.array_equal(d_ids.download(np.uint64, max(n, 1))[:n], exp_ids), (name, form)
                n2 = lay.unpack_selected(d_words, d_bm, d_out)   # without ids
                assert n2 == n and np.array_equal(d_out.download(dtype, max(n, 1))[:n], exp_vals), (name, form)


@gpu
@pytest.mark.parametrize("dtype", [np.uint64, np.int32, np.uint16, np.int8])
def test_gather_forms_agree_on_ragged_segments(adac, oracle, gpu_ctx, dtype):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(70 + 8 * dtype.itemsize)
    lay, d_words, counts, segs, offs, span = ragged_gather_column(adac, oracle, gpu_ctx, rng, dtype)
    check_gather_forms(adac, gpu_ctx, lay, d_words, dtype, counts, segs, offs, span, rng)


@gpu
@pytest.mark.parametrize("dtype", [np.uint64, np.int32, np.uint16, np.uint8])
def test_gather_forms_agree_on_many_tiny_segments(adac, oracle, gpu_ctx, dtype):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(4242 + dtype.itemsize)
    lay, d_words, counts, segs, offs, span = many_groups_column(adac, oracle, gpu_ctx, rng, dtype)
    check_gather_forms(adac, gpu_ctx, lay, d_words, dtype, counts, segs, offs, span, rng)


# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_knobs_are_back_at_their_defaults(adac, oracle, gpu_ctx):
    """After the module: the first test's default-knob encode gives the same bytes again, and a stamped encode spreads
    over the device (num_cus is 0) — stamps themselves off again afterwards."""
    dtype = np.dtype(np.uint64)
    col = walk_column(dtype, walk_kinds(dtype)[:12], limit_rows=3000)
    again = ordered(adac, oracle, gpu_ctx, dtype, col)[:2]
    first = _first.get("default", again)
    assert again[0] == first[0] and np.array_equal(again[1], first[1])
    rng = np.random.default_rng(17)
    counts = np.full(300, 20000, dtype=np.uint32)
    segs = [make_values(rng, dtype, 20000, 13) for _ in range(300)]
    try:
        adac.set_tuning("encode_stamps", 1)
        run_encode_decode(adac, oracle, gpu_ctx, dtype, counts, segs)    # (8-byte type: the single pass by default)
    finally:
        adac.set_tuning("encode_stamps", 0)
    assert len(set(stamp_places(adac, 300).tolist())) > 2
