"""adac_reencode / adac_analyze_packed / adac_repack over the whole (old_w, new_w) plane of every type
(tests/repack_cases.py; what the plane reaches is asserted on the CPU by tests/test_repack_census.py).

The bar is the one of test_gpu_repack.py — the destination is bit-identical to the oracle's direct encode of the values
the source decodes to (oracle_encode: orc_analyze_flat, the two width rules, orc_pack_flat) — on more of it: the
destination's min/max scratch, its stored min, every word of its arena (the words no segment owns stay zero), and the
decode through the destination.  No tolerances: this is integer work.

  a. adac_reencode over the plane, source and destination under the same rule, both rules;
  b. across the rules (RULE_APPEND's sign-extended extrema <-> RULE_RECOMPACT's zero-extended ones), on the plane and on
     a small signed column whose min representation changes;
  c. adac_repack alone into descriptors written by the test: the only way to a destination wider than the values need,
     or wider than the source (repack_run_w's t / nd bookkeeping at every new_w against every compile-time old_w);
  d. NULLs: a validity mask over gapped value offsets, arbitrary fields in the source's NULL slots, both rules; the
     result also equals adac_encode of the same values and mask, the all-NULL segment under RULE_APPEND included;
  e. the LDS-staged form (templated_scan = 0) writes the same bytes as the default;
  f. several scan groups per segment (scan_tiles_per_wg = 2) with several stages each.
The 2^31-bit gate of the register walk is test_gpu_big_segments.py's and is not repeated here."""
import numpy as np
import pytest

import repack_cases as rc
from test_gpu_parity import U64, oracle_encode, run_encode_decode

pytestmark = pytest.mark.gpu

RULES = (0, 1)                                   # ADAC_RULE_APPEND, ADAC_RULE_RECOMPACT
_cases, _sources, _defaults = {}, {}, {}         # built once per module run; the device buffers live with gpu_ctx


def case_of(dtype, kind="plane"):
    key = (np.dtype(dtype), kind)
    if key not in _cases:
        _cases[key] = (rc.make_group_case(dtype) if kind == "groups" else rc.make_case(dtype, null_variant=kind == "nulls"))
    return _cases[key]


def offsets_of(case):
    if case.val_offs is not None:
        return case.val_offs
    return np.concatenate([[0], np.cumsum(case.counts)[:-1]]).astype(np.uint64)


def span_of(case):
    return int(offsets_of(case)[-1]) + int(case.counts[-1])


def source_of(adac, orc, ctx, dtype, kind, rule):
    """The source of a case under `rule`: the wide values encoded (run_encode_decode holds that against the oracle), every
    segment at exactly its old_w; then the arena rewritten on the host at the OLD widths and mins with the narrow
    values — what in-place updates leave behind — and decoded once to see that it holds them."""
    key = (np.dtype(dtype), kind, rule)
    if key in _sources:
        return _sources[key]
    case = case_of(dtype, kind)
    src, d_src, _, sd, _ = run_encode_decode(adac, orc, ctx, case.dtype, case.counts, case.wide, rule, False, None,
                                             case.val_offs)
    tb = 8 * case.dtype.itemsize
    assert sd["width"].tolist() == case.old_w
    assert [bool(f & adac.SEG_PACKED) for f in sd["flags"]] == [w < tb for w in case.old_w]
    host = np.zeros(src.max_arena_words, dtype=np.uint64)
    for s, v in enumerate(case.narrow):
        packed = case.old_w[s] < tb
        ws = orc.pack_flat(v, int(sd["min"][s]) if packed else U64, case.old_w[s])
        off = int(sd["word_off"][s])
        host[off:off + len(ws)] = ws
    d_src.upload(host)
    d_out = ctx.alloc(span_of(case) * case.dtype.itemsize + 64).zero()
    src.unpack(d_src, d_out)
    got = d_out.download(case.dtype, span_of(case))
    for s, (v, o) in enumerate(zip(case.narrow, offsets_of(case))):
        assert np.array_equal(got[int(o):int(o) + len(v)], v), "rewritten source, segment %d" % s
    _sources[key] = (case, src, d_src)
    return _sources[key]


def new_dst(adac, ctx, case):
    dst = adac.Layout(ctx, case.dtype, case.counts, case.val_offs)
    return dst, ctx.alloc(dst.max_arena_words * 8 + 16).zero()


def check_reencoded(adac, orc, ctx, case, segs, dst, d_dst, rule, validity=None, valid=None):
    """dst against the oracle's direct encode of `segs`: descriptors, min/max, the whole arena, and the decode."""
    offs = offsets_of(case)
    exp = oracle_encode(orc, segs, rule, False, validity, offs)
    descs, mm = dst.get_descs(), dst.get_minmax()
    words = d_dst.download(np.uint64, dst.max_arena_words)
    arena = np.zeros(dst.max_arena_words, dtype=np.uint64)
    woff = 0
    for s, (mn, mx, w, packed, ew) in enumerate(exp):
        d = descs[s]
        what = "segment %d (%d -> %d)" % (s, case.old_w[s], case.new_w[s])
        assert (int(mm[s, 0]), int(mm[s, 1])) == (mn, mx), "min/max of " + what
        assert int(d["width"]) == w and bool(d["flags"] & adac.SEG_PACKED) == packed, "width of " + what
        assert int(d["word_off"]) == woff, what
        if packed:
            assert int(d["min"]) == adac.stored_min(mn, mx, w), "stored min of " + what
        assert np.array_equal(words[woff:woff + len(ew)], ew), "words of " + what
        arena[woff:woff + len(ew)] = ew
        woff += adac.arena_words(len(segs[s]), w)
    assert np.array_equal(words, arena), "words outside the segments' packed words"
    span = span_of(case)
    d_out = ctx.alloc(span * case.dtype.itemsize + 64).zero()
    dst.unpack(d_dst, d_out)
    got = d_out.download(case.dtype, span)
    for s, (v, o) in enumerate(zip(segs, offs)):
        ok = slice(None) if valid is None else valid[int(o):int(o) + len(v)]
        assert np.array_equal(got[int(o):int(o) + len(v)][ok], v[ok]), "decode of segment %d" % s
    return words, descs, mm


def reencode_plane(adac, orc, ctx, dtype, src_rule, dst_rule, check=True):
    case, src, d_src = source_of(adac, orc, ctx, dtype, "plane", src_rule)
    dst, d_dst = new_dst(adac, ctx, case)
    src.reencode(d_src, dst, d_dst, None, dst_rule, False)
    if check:
        return check_reencoded(adac, orc, ctx, case, case.narrow, dst, d_dst, dst_rule)
    return d_dst.download(np.uint64, dst.max_arena_words), dst.get_descs(), dst.get_minmax()


def repack_into(adac, orc, ctx, case, src, d_src, check=True):
    """adac_repack alone: the destination's descriptors are the generated (new_w, dst min), PACKED iff new_w < tb, at
    the 16-word-aligned prefix offsets of adac.arena_words."""
    tb = 8 * case.dtype.itemsize
    dst, d_dst = new_dst(adac, ctx, case)
    descs = dst.get_descs()
    woff = 0
    for s, w in enumerate(case.new_w):
        descs["word_off"][s], descs["min"][s], descs["width"][s] = woff, case.dst_min[s], w
        descs["flags"][s] = adac.SEG_PACKED if w < tb else 0
        woff += adac.arena_words(int(case.counts[s]), w)
    assert woff <= dst.max_arena_words
    dst.set_descs(descs)
    src.repack(d_src, dst, d_dst)
    words = d_dst.download(np.uint64, dst.max_arena_words)
    if not check:
        return words, dst.get_descs()
    arena = np.zeros(dst.max_arena_words, dtype=np.uint64)
    for s, v in enumerate(case.narrow):
        ew = orc.pack_flat(v, case.dst_min[s], case.new_w[s])
        off = int(descs["word_off"][s])
        assert np.array_equal(words[off:off + len(ew)], ew), "words of segment %d (%d -> %d, %d rows)" % (
            s, case.old_w[s], case.new_w[s], len(v))
        arena[off:off + len(ew)] = ew
    assert np.array_equal(words, arena), "words outside the segments' packed words"
    total = int(case.counts.sum())
    d_out = ctx.alloc(total * case.dtype.itemsize + 64).zero()
    dst.unpack(d_dst, d_out)
    assert np.array_equal(d_out.download(case.dtype, total), np.concatenate(case.narrow))
    return words, dst.get_descs()


def default_of(key, run):
    if key not in _defaults:
        _defaults[key] = run()
    return _defaults[key]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dtype", rc.ALL)
def test_reencode_plane_same_rule(adac, oracle, gpu_ctx, dtype, rule):
    """(a) Every pair, source and destination under one rule."""
    got = reencode_plane(adac, oracle, gpu_ctx, dtype, rule, rule)
    _defaults.setdefault((np.dtype(dtype), "reencode", rule), got)


@pytest.mark.parametrize("src_rule", RULES)
@pytest.mark.parametrize("dtype", rc.ALL)
def test_reencode_plane_across_rules(adac, oracle, gpu_ctx, dtype, src_rule):
    """(b) A column appended under one rule is re-compacted under the other: the extrema change between sign- and
    zero-extension (the `sx` conversions at the end of k_analyze_packed_g's register path), the stored min of an
    all-negative signed segment with them."""
    reencode_plane(adac, oracle, gpu_ctx, dtype, src_rule, 1 - src_rule)


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.int16, np.int8])
def test_reencode_signed_column_across_rules(adac, oracle, gpu_ctx, dtype):
    """(b) All-negative segments (packed under both rules; min 0xff..f80 under RULE_APPEND, 0x80 under RULE_RECOMPACT for
    an int8) and segments in [-k, k] (unpacked under both), re-encoded in both directions."""
    dtype = np.dtype(dtype)
    counts, segs = rc.cross_rule_column(dtype)
    nneg = len(segs) - 3
    for src_rule in RULES:
        src, d_src, _, sd, _ = run_encode_decode(adac, oracle, gpu_ctx, dtype, counts, segs, src_rule)
        assert all(sd["flags"][:nneg] & adac.SEG_PACKED) and not any(sd["flags"][nneg:] & adac.SEG_PACKED)
        case = rc.Case(dtype, counts, sd["width"].tolist(), sd["width"].tolist(), *([None] * 12))
        dst, d_dst = new_dst(adac, gpu_ctx, case)
        src.reencode(d_src, dst, d_dst, None, 1 - src_rule, False)
        _, dd, _ = check_reencoded(adac, oracle, gpu_ctx, case, segs, dst, d_dst, 1 - src_rule)
        assert dd["width"].tolist() == sd["width"].tolist()
        if dtype.itemsize < 8:                       # sign- against zero-extended: another stored min, the same words
            assert all(dd["min"][:nneg] != sd["min"][:nneg])


@pytest.mark.parametrize("dtype", rc.ALL)
def test_repack_plane(adac, oracle, gpu_ctx, dtype):
    """(c) adac_repack into every destination width, from every source width."""
    case, src, d_src = source_of(adac, oracle, gpu_ctx, dtype, "plane", adac.RULE_APPEND)
    got = repack_into(adac, oracle, gpu_ctx, case, src, d_src)
    _defaults.setdefault((np.dtype(dtype), "repack"), got)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dtype", rc.ALL)
def test_reencode_with_nulls(adac, oracle, gpu_ctx, dtype, rule):
    """(d) The NULL slots of the source hold arbitrary fields and must not count: the sink takes NullValue<T> for them.
    Expected: the oracle's encode of the decoded values under the mask — and adac_encode of the same values and mask,
    byte for byte, the segments without a valid row under RULE_APPEND included (their min stays UINT64_MAX and nothing
    is subtracted: succinct.cpp:276-292)."""
    case, src, d_src = source_of(adac, oracle, gpu_ctx, dtype, "nulls", rule)
    d_valid = gpu_ctx.upload(case.validity)
    dst, d_dst = new_dst(adac, gpu_ctx, case)
    src.reencode(d_src, dst, d_dst, d_valid, rule, False)
    words, descs, mm = check_reencoded(adac, oracle, gpu_ctx, case, case.narrow, dst, d_dst, rule, case.validity, case.valid)
    enc, d_enc, _, ed, _ = run_encode_decode(adac, oracle, gpu_ctx, case.dtype, case.counts, case.narrow, rule, False,
                                             case.validity, case.val_offs)
    assert np.array_equal(descs, ed)
    assert np.array_equal(mm, enc.get_minmax())
    assert np.array_equal(words, d_enc.download(np.uint64, enc.max_arena_words))
    if rule == adac.RULE_APPEND:
        offs = offsets_of(case)
        empty = [s for s, (o, c) in enumerate(zip(offs, case.counts)) if not case.valid[int(o):int(o) + int(c)].any()]
        assert empty and all(int(mm[s, 0]) == U64 and int(mm[s, 1]) == 0 for s in empty)


@pytest.mark.parametrize("dtype", rc.ALL)
def test_generic_form_equals_register_form(adac, oracle, gpu_ctx, dtype):
    """(e) templated_scan = 0: the LDS-staged form of both kernels on the same sources; words, descriptors and min/max
    byte-identical to the default's (which (a) and (c) hold against the oracle)."""
    dtype = np.dtype(dtype)
    case, src, d_src = source_of(adac, oracle, gpu_ctx, dtype, "plane", adac.RULE_APPEND)
    for rule in RULES:
        source_of(adac, oracle, gpu_ctx, dtype, "plane", rule)
        default_of((dtype, "reencode", rule), lambda: reencode_plane(adac, oracle, gpu_ctx, dtype, rule, rule))
    default_of((dtype, "repack"), lambda: repack_into(adac, oracle, gpu_ctx, case, src, d_src))
    try:
        adac.set_tuning("templated_scan", 0)
        generic = {(dtype, "reencode", rule): reencode_plane(adac, oracle, gpu_ctx, dtype, rule, rule, check=False)
                   for rule in RULES}
        generic[(dtype, "repack")] = repack_into(adac, oracle, gpu_ctx, case, src, d_src, check=False)
    finally:
        adac.set_tuning("templated_scan", 1)
    for key, got in generic.items():
        for a, b in zip(got, _defaults[key]):
            assert a.tobytes() == b.tobytes(), key


@pytest.mark.parametrize("dtype", rc.ALL)
def test_several_groups_and_stages(adac, oracle, gpu_ctx, dtype):
    """(f) Segments of 5 tiles + 37 rows at scan_tiles_per_wg = 2: three scan groups each, the last partial; the
    register walk at source widths 5, 13 and 32, the staged form at 3 -> 2 and (8-byte types) 40 -> 33."""
    case, src, d_src = source_of(adac, oracle, gpu_ctx, dtype, "groups", adac.RULE_APPEND)
    try:
        adac.set_tuning("scan_tiles_per_wg", rc.GROUP_TILES_PER_WG)
        dst, d_dst = new_dst(adac, gpu_ctx, case)
        src.reencode(d_src, dst, d_dst)
        repacked = repack_into(adac, oracle, gpu_ctx, case, src, d_src, check=False)
    finally:
        adac.set_tuning("scan_tiles_per_wg", 0)
    check_reencoded(adac, oracle, gpu_ctx, case, case.narrow, dst, d_dst, adac.RULE_APPEND)
    again = repack_into(adac, oracle, gpu_ctx, case, src, d_src)     # default grouping, held against the oracle
    for a, b in zip(repacked, again):
        assert a.tobytes() == b.tobytes()


def test_knobs_are_back_at_their_defaults(adac, oracle, gpu_ctx):
    """After the module: the default call gives the first default call's bytes again.  (Both forms and every grouping
    write the same bytes, so this holds the calls, not the knobs' values; each test above restores its knob in a
    `finally`.)"""
    dtype = np.dtype(np.uint32)
    first = default_of((dtype, "reencode", 0), lambda: reencode_plane(adac, oracle, gpu_ctx, dtype, 0, 0))
    again = reencode_plane(adac, oracle, gpu_ctx, dtype, 0, 0, check=False)
    for a, b in zip(again, first):
        assert a.tobytes() == b.tobytes()
