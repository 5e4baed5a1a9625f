"""What the columns of tests/repack_cases.py reach in k_analyze_packed_g and k_repack_g, asserted on the CPU through the
mirror of the kernels' predicates: a generator that stops reaching a form, a size, a position or a stage count fails
here, without a GPU.  Every statement is exact — a condition on the generator, not a share that may be missed.

The 8-byte plane is NOT thinned (repack_cases.THIN_8_BYTE_PLANE): all 4096 pairs run, plus the extra old_w -> 32 segments
that give every source width of the register walk a second stage (see the module's note)."""
import collections

import numpy as np
import pytest

import repack_cases as rc

REG, ST, ST32, ST64 = "register", "staged", "staged32", "staged64"


@pytest.fixture(scope="module", params=rc.ALL, ids=lambda d: np.dtype(d).name)
def dtype(request):
    return np.dtype(request.param)


@pytest.fixture(scope="module")
def plane(dtype):
    case = rc.make_case(dtype)
    paths = [rc.path_of(case.dtype.itemsize, o, n, int(c)) for o, n, c in zip(case.old_w, case.new_w, case.counts)]
    return case, paths


@pytest.fixture(scope="module")
def nulls(dtype):
    case = rc.make_case(dtype, null_variant=True)
    paths = [rc.path_of(case.dtype.itemsize, o, n, int(c), validity=True)
             for o, n, c in zip(case.old_w, case.new_w, case.counts)]
    return case, paths


def test_the_mirror_on_known_points():
    """Figures worked out by hand from the kernel's lines."""
    assert rc.tile_values(8) == 2048 and rc.tile_values(1) == 16384
    assert rc.repack_stage_rows(4, 8, 8, REG) == 16384 and rc.repack_stage_rows(8, 5, 32, REG) == 4096
    assert rc.repack_stage_rows(8, 9, 31, REG) == 4224                        # (131072 / 31) & ~127
    assert rc.repack_stage_rows(8, 64, 64, ST64) == 1024 and rc.repack_stage_rows(8, 40, 33, ST64) == 1536
    assert rc.repack_stage_rows(1, 3, 2, ST32) == 20480 and rc.repack_stage_rows(8, 3, 2, ST32) == 21504
    assert rc.analyze_stage_rows(8, 64, ST) == 2048 and rc.analyze_stage_rows(8, 3, ST) == 21 * 2048
    assert rc.analyze_stage_rows(4, 8, REG) is None
    assert rc.scan_groups(8, 5 * 2048 + 37, 2) == [(0, 4096), (4096, 4096), (8192, 2085)]
    assert rc.scan_groups(8, 2 * 2048 + 37) == [(0, 4133)] and rc.scan_groups(1, 0) == []
    assert rc.scan_groups(1, 5 * 16384) == [(0, 49152), (49152, 32768)]       # 5 tiles, 4 per group: dealt 3 + 2
    assert rc.repack_form(8, 32, 33, 100) == ST64 and rc.repack_form(8, 32, 32, 100) == REG
    assert rc.repack_form(8, 33, 32, 100) == ST32 and rc.repack_form(4, 3, 32, 100) == ST32
    assert rc.repack_form(4, 8, 8, 100, validity=True) == ST32 and rc.repack_form(4, 8, 8, 100, templated=False) == ST32
    assert rc.analyze_form(4, 8, 1 << 28) == ST and rc.analyze_form(4, 8, (1 << 28) - 1) == REG   # the 2^31-bit gate
    assert rc.stages_of(4133, 4096) == (2, True) and rc.stages_of(4096, 4096) == (1, False)


def test_every_pair_is_present_exactly_once(plane):
    case, _ = plane
    tb = 8 * case.dtype.itemsize
    pairs = [(o, n) for o, n, x in zip(case.old_w, case.new_w, case.extra) if not x]
    assert len(pairs) == tb * tb and set(pairs) == {(o, n) for o in range(1, tb + 1) for n in range(1, tb + 1)}
    extras = [(o, n) for o, n, x in zip(case.old_w, case.new_w, case.extra) if x]
    assert extras == ([(o, 32) for o in range(4, 33) if o % 4 != 3] if tb == 64 else [])
    sizes = [rc.size_rows(case.dtype.itemsize, 3 if x else rc.pair_size(o, n))
             for o, n, x in zip(case.old_w, case.new_w, case.extra)]
    assert case.counts.tolist() == sizes


def test_every_width_meets_every_size_position_and_frame(plane):
    case, _ = plane
    tb = 8 * case.dtype.itemsize
    seen_old, seen_new, frames = collections.defaultdict(set), collections.defaultdict(set), set()
    for o, n, size, pos, frame, x in zip(case.old_w, case.new_w, case.size, case.position, case.frame, case.extra):
        if not x:
            seen_old[o].add((size, pos))
            seen_new[n].add((size, pos))
            frames.add((frame, pos))
    cells = {(s, p) for s in range(4) for p in range(3)}
    for w in range(1, tb + 1):
        if tb >= 16:                                  # 12 cells need 12 pairs: a 1-byte type has 8 per width
            assert seen_old[w] == cells and seen_new[w] == cells, w
        assert {s for s, _ in seen_old[w]} == set(range(4)) and {s for s, _ in seen_new[w]} == set(range(4)), w
        assert {p for _, p in seen_old[w]} == set(range(3)) and {p for _, p in seen_new[w]} == set(range(3)), w
    assert frames == {(f, p) for f in range(3) for p in range(3)}


def test_the_values_are_what_the_rotations_say(plane):
    """Both ends of the narrow range are present, it lies where its position says, inside the old frame; the old frame
    never wraps the type and a signed one spans the sign change only at old_w = tb."""
    case, _ = plane
    tb = 8 * case.dtype.itemsize
    udt = np.dtype("u%d" % case.dtype.itemsize)
    wider = 0
    for s, (o, n, bits, pos, frame, base) in enumerate(zip(case.old_w, case.new_w, case.bits, case.position, case.frame,
                                                           case.base)):
        wide, narrow = case.wide[s].view(udt), case.narrow[s].view(udt)
        assert (int(wide.min()), int(wide.max())) == (base, base + (1 << o) - 1) and base + (1 << o) <= 1 << tb
        lo, hi = int(narrow.min()), int(narrow.max())
        assert hi - lo == (1 << bits) - 1 and bits == min(o, n) - ((o + n) % 3 == 0)
        assert base <= lo and hi <= base + (1 << o) - 1
        if pos == 0:
            assert lo == base
        elif pos == 1:
            assert hi == base + (1 << o) - 1
        else:                                             # an odd offset wherever the frame has room for one
            assert (lo - base) % 2 == 1 or bits == o
        wider += bits < n
        if o < tb:
            if frame == 1:
                assert base + (1 << o) == 1 << tb
            if case.dtype.kind == "i":
                assert (base >= 1 << (tb - 1)) == (frame != 0) and (base + (1 << o) - 1 >= 1 << (tb - 1)) == (frame != 0)
        lowered = case.dst_min[s] == rc.U64 - ((1 << n) - 1) and lo == rc.U64
        assert case.dst_min[s] == (rc.U64 if n == tb else lo) or lowered
    assert wider >= len(case.old_w) // 3                  # destinations genuinely wider than the values need


def test_every_cell_the_predicates_allow_is_reached(plane):
    """(form of analyze) x (form of repack) x size x position: the cells the predicates allow are non-empty, the others
    empty.  Without a mask the register walks go together (analyze's condition is repack's without new_w <= 32), so
    register/staged32 and staged/register cannot occur; the 64-bit emission needs new_w > 32: an 8-byte type."""
    case, paths = plane
    tb = 8 * case.dtype.itemsize
    forms = {(REG, REG), (ST, ST32)} | ({(REG, ST64), (ST, ST64)} if tb == 64 else set())
    cells = collections.Counter((p.analyze, p.repack, size, pos)
                                for p, size, pos, x in zip(paths, case.size, case.position, case.extra) if not x)
    assert set(cells) == {(a, r, s, p) for a, r in forms for s in range(4) for p in range(3)}
    assert all(p.groups == 1 for p in paths)              # (several groups: the column of make_group_case)


def test_the_register_walk_at_every_source_width(plane):
    """Every source width 4..32 reaches repack_run_w with a run of one stage and with a run of more than one, the
    last one partial (the 8-byte types through the extra segments); analyze_run_w takes each run whole."""
    case, paths = plane
    tb = 8 * case.dtype.itemsize
    one, more = set(), set()
    for o, p in zip(case.old_w, paths):
        if p.repack == REG:
            assert p.analyze == REG and p.analyze_stages == 1
            (one if p.repack_stages == 1 else more).add(o)
            assert p.repack_stages == 1 or p.repack_partial
    assert one == more == set(range(4, min(tb, 32) + 1))
    # the staged forms too: a run of several stages in each emission the type has.  The staged min/max pass meets
    # one only under templated_scan = 0 for the 2- and 4-byte types (their unmasked staged sources are 1..3 bits wide:
    # a stage of 5 tiles or more), which is how test_generic_form_equals_register_form runs the plane
    generic = [rc.path_of(case.dtype.itemsize, o, n, int(c), templated=False)
               for o, n, c in zip(case.old_w, case.new_w, case.counts)]
    staged = collections.defaultdict(set)
    for p, q in zip(paths, generic):
        if p.repack != REG:
            staged[p.repack].add(min(p.repack_stages, 2))
        if p.analyze == ST:
            staged[ST].add(min(p.analyze_stages, 2))
        staged["generic"].add(min(q.analyze_stages, 2))
    assert staged[ST32] == {1, 2} and (tb < 64 or staged[ST64] == {1, 2})
    assert staged[ST] == ({1, 2} if tb in (8, 64) else {1}) and staged["generic"] == {1, 2}


def test_both_emissions_with_and_without_a_mask(plane, nulls):
    case, paths = plane
    ncase, npaths = nulls
    tb = 8 * case.dtype.itemsize
    want = {ST32, ST64} if tb == 64 else {ST32}
    assert {p.repack for p in paths} - {REG} == want
    assert {p.repack for p in npaths} == want and {p.analyze for p in npaths} == {ST}    # a mask: never the register walk
    generic = [rc.path_of(case.dtype.itemsize, o, n, int(c), templated=False)
               for o, n, c in zip(case.old_w, case.new_w, case.counts)]
    assert {p.repack for p in generic} == want and {p.analyze for p in generic} == {ST}
    keep = set(range(1, 9)) if tb == 8 else {w for w in rc.NULL_WIDTHS + (tb,) if w <= tb}
    assert set(zip(ncase.old_w, ncase.new_w)) == {(o, n) for o in keep for n in keep}
    assert len(ncase.old_w) == len(keep) ** 2


def test_the_null_variant_masks(nulls):
    case, _ = nulls
    K = 16 // case.dtype.itemsize
    kinds = collections.Counter()
    phases = set()
    end = 0
    for s, (o, c) in enumerate(zip(case.val_offs, case.counts)):
        o, c = int(o), int(c)
        assert o > end or s == 0 and o > 0                # a non-zero gap before every segment
        assert o % 64 == (37 * s + 1) % 64
        end = o + c
        ok = case.valid[o:o + c]
        kinds["none"] += not ok.any()
        kinds["all"] += bool(ok.all())
        kinds["some"] += bool(ok.any() and not ok.all())
        phases |= {(o + b) % 64 for b in range(0, c, K)}   # the sink's validity_window calls: one per chunk of K rows
    assert kinds["none"] >= 1 and kinds["all"] >= 1 and kinds["some"] >= 1
    assert phases == set(range(64))
    assert len(case.valid) == end and len(case.validity) * 64 >= end + 64


def test_the_group_column(dtype):
    """5 tiles + 37 rows at scan_tiles_per_wg = 2: three groups, the last partial; the register walk and the staged
    form both occur, and some group takes more than one stage."""
    case = rc.make_group_case(dtype)
    size, tb = case.dtype.itemsize, 8 * case.dtype.itemsize
    assert list(zip(case.old_w, case.new_w)) == [(o, min(n, tb)) for o, n in rc.GROUP_PAIRS if o <= tb]
    paths = [rc.path_of(size, o, n, int(c), tiles_per_wg=rc.GROUP_TILES_PER_WG)
             for o, n, c in zip(case.old_w, case.new_w, case.counts)]
    tile = rc.tile_values(size)
    for c, p in zip(case.counts, paths):
        assert int(c) == 5 * tile + 37 and p.groups == 3
        assert rc.scan_groups(size, int(c), rc.GROUP_TILES_PER_WG)[-1] == (4 * tile, tile + 37)
    assert {p.repack for p in paths} >= {REG, ST32} and (tb < 64 or paths[-1].repack == ST64)
    assert max(p.repack_stages for p in paths) > 1


def test_the_cross_rule_column(dtype):
    if dtype.kind != "i":
        return
    counts, segs = rc.cross_rule_column(dtype)
    assert counts.tolist() == [len(v) for v in segs]
    assert all(int(v.max()) < 0 for v in segs[:-3]) and any(int(v.max()) == -1 for v in segs[:-3])
    assert [(int(v.min()), int(v.max())) for v in segs[-3:]] == [(-k, k) for k in (1, 5, np.iinfo(dtype).max)]
    forms = {rc.analyze_form(dtype.itemsize, w, int(c)) for w, c in
             zip([int(v.view("u%d" % dtype.itemsize).max() - v.view("u%d" % dtype.itemsize).min()).bit_length()
                  for v in segs[:-3]], counts)}
    assert forms == {REG, ST}
