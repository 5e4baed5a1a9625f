"""Host mirror of the device rule "which kernel form takes this scan group" (no device code, no library).

The product scans choose per scan group of `a` between a register walk ("fast") and a staged kernel ("generic").
The rule is product_fast_eligible (csrc/adac_sum_product.inl), group_product_rw_eligible (csrc/adac_group_product.inl)
and group_product3_rw_eligible / group_q1_rw_eligible, which chain onto it.  Read as one rule over N value columns, a
scan group is fast when
  * 4 <= w_a <= 32, and 1 <= w <= 32 for every other value column;
  * count * w < 2^31 bits for every value column;
  * value = field + frame holds for every field of every value column (frame());
  * grouped forms only: ngroups + 1 <= 8; 0 <= frame and frame + 2^w - 1 < 2^32 for every value column; and the key
    column passes keys_ok().
Descriptors are rows of SEGMENT_DESC_DTYPE (Layout.get_descs()); a type is (size in bytes, signed).  Every function
returns {"fast": scan groups of a, "generic": scan groups of a} with the default grouping of ensure_scan_groups.

The compare scan (k_scan_compare, csrc/adac_scan_compare.inl) has a third form in front of the two: "header", when both
columns have a frame() and the intervals [frame, frame + 2^w - 1] are disjoint as mathematical integers (or both are
single values), so that the descriptors alone decide every row.  compare_form_groups names the form per segment pair.

The member scans (k_scan_member / k_scan_member_build, csrc/adac_scan_member.inl) choose a reader and a set access per
segment from the descriptor, the type and the domain (set_base, set_bits): member_form_groups mirrors member_plan.

The grouped SUM / COUNT by a dense key (k_group_dense, csrc/adac_group_dense.inl) chooses a reader and an accumulator
per key segment the same way, the walk also asking the value column: dense_form_groups mirrors dense_plan.

The grouped SUM / COUNT by a code looked up through a dense key (k_group_mapped, csrc/adac_group_mapped.inl) takes the
same readers and, instead of the window, an on-chip slice of the map: mapped_form_groups mirrors mapped_plan.

The grouped SUM(a * b) through the map (k_group_mapped_product, csrc/adac_group_mapped_product.inl) asks BOTH value
columns before it walks: mapped_product_form_groups mirrors mapped_product_plan.
"""
from itertools import repeat

NO_MIN = 0xFFFFFFFFFFFFFFFF
TILE_BYTES = 16384
TILES_PER_SCAN_GROUP = {8: 12, 4: 6, 2: 8, 1: 4}   # by the type size of a


def has_min(d):
    return bool(int(d["flags"]) & 1) and int(d["min"]) != NO_MIN


def frame(d, size, signed):
    """product_frame: the widened frame of reference when value = field + frame for every field, else None"""
    tb = 8 * size
    tmask, sbit = (1 << tb) - 1, (1 << (tb - 1)) if signed else 0
    if has_min(d):
        bmin = (int(d["min"]) & tmask) ^ sbit
        return bmin - sbit if bmin + (1 << int(d["width"])) - 1 <= tmask else None
    return 0 if sbit == 0 else None


def value_ok(d, kind, min_width, grouped):
    """One value column's side of the rule; min_width is 4 for a and 1 for the others."""
    w = int(d["width"])
    if not (min_width <= w <= 32 and int(d["count"]) * w < 2 ** 31):
        return False
    m = frame(d, *kind)
    return m is not None and (not grouped or (0 <= m and m + (1 << w) - 1 < 2 ** 32))


def keys_ok(d, k_size, ngroups):
    """The key side of group_product_rw_eligible: at most 8 bits, the keys do not wrap in their type, and all keys of
    the segment fit a byte or all of them are >= ngroups."""
    wk, kmask = int(d["width"]), (1 << (8 * k_size)) - 1
    if wk > 8:
        return False
    kadd = (int(d["min"]) & kmask) if has_min(d) else 0
    top = kadd + (1 << wk) - 1
    return top <= kmask and (top <= 255 or kadd >= ngroups)


def form_groups(value_descs, kinds, descs_k=None, ngroups=None, k_size=1):
    """The rule over the value columns value_descs (a first) of types kinds; grouped when descs_k is given."""
    grouped = descs_k is not None
    size_a = kinds[0][0]
    tile, per = TILE_BYTES // size_a, TILES_PER_SCAN_GROUP[size_a]
    out = {"fast": 0, "generic": 0}
    for *ds, dk in zip(*value_descs, descs_k if grouped else repeat(None)):
        ntiles = (int(ds[0]["count"]) + tile - 1) // tile
        if ntiles == 0:
            continue
        fast = all(value_ok(d, kind, 1 if i else 4, grouped) for i, (d, kind) in enumerate(zip(ds, kinds)))
        if fast and grouped:
            fast = ngroups + 1 <= 8 and keys_ok(dk, k_size, ngroups)
        out["fast" if fast else "generic"] += (ntiles + per - 1) // per
    return out


def product_form_groups(descs_a, descs_b, type_size=4, signed=True):
    """adac_scan_sum_product (k_scan_product): product_fast_eligible; both columns of one type."""
    return form_groups((descs_a, descs_b), [(type_size, signed)] * 2)


def group_product_form_groups(descs_a, descs_b, descs_k, ngroups, a_type=(4, True), b_type=(4, True), k_size=1):
    """adac_scan_group_sum_product: group_product_rw_eligible."""
    return form_groups((descs_a, descs_b), (a_type, b_type), descs_k, ngroups, k_size)


def group_product3_form_groups(descs_a, descs_b, descs_c, descs_k, ngroups, a_type=(4, True), b_type=(4, True),
                               c_type=(4, True), k_size=1):
    """adac_scan_group_sum_product3: group_product3_rw_eligible (for c what holds for b)."""
    return form_groups((descs_a, descs_b, descs_c), (a_type, b_type, c_type), descs_k, ngroups, k_size)


def group_q1_form_groups(descs_a, descs_b, descs_c, descs_q, descs_k, ngroups, a_type=(4, True), b_type=(4, True),
                         c_type=(4, True), q_type=(4, True), k_size=1):
    """adac_scan_group_sum_q1: group_q1_rw_eligible (for q what holds for c)."""
    return form_groups((descs_a, descs_b, descs_c, descs_q), (a_type, b_type, c_type, q_type), descs_k, ngroups, k_size)


def compare_form_groups(descs_a, descs_b, a_type=(4, True), b_type=(4, True)):
    """adac_scan_select_compare / adac_scan_count_compare (k_scan_compare): compare_plan, per segment pair "header",
    "fast" or "generic" (every scan group of a segment takes the same form); None for a segment without rows."""
    out = []
    for da, db in zip(descs_a, descs_b):
        if int(da["count"]) == 0:
            out.append(None)
            continue
        ma, mb = frame(da, *a_type), frame(db, *b_type)
        form = "generic"
        if ma is not None and mb is not None:
            sa, sb = (1 << int(da["width"])) - 1, (1 << int(db["width"])) - 1
            if ma + sa < mb or mb + sb < ma or (sa == 0 and sb == 0):
                form = "header"
            elif value_ok(da, a_type, 4, False) and value_ok(db, b_type, 1, False):
                form = "fast"
        out.append(form)
    return out


MEMBER_SLICE_BITS = 65536   # kMemberSliceBits


def member_form_groups(descs, type, set_base, set_bits):
    """adac_scan_select_member / adac_scan_count_member / adac_scan_build_member: member_plan, per segment "header",
    "walk-slice", "walk-direct", "staged-slice" or "staged-direct" (every scan group of a segment takes the same form);
    None for a segment without rows.  type: (size in bytes, signed); set_base: a bit pattern of the type."""
    size, signed = type
    sbit = (1 << (8 * size - 1)) if signed else 0
    dlo = (int(set_base) ^ sbit)            # biased by the sign bit every interval is one of unsigned numbers
    dhi = dlo + int(set_bits) - 1
    out = []
    for d in descs:
        if int(d["count"]) == 0:
            out.append(None)
            continue
        m = frame(d, size, signed)
        if m is None:
            out.append("staged-direct")
            continue
        bmin = m + sbit
        btop = bmin + (1 << int(d["width"])) - 1
        if btop < dlo or dhi < bmin:
            out.append("header")
            continue
        lo, hi = max(bmin - dlo, 0), min(btop, dhi) - dlo + 1   # set bits [lo, hi) are what the segment can reach
        reader = "walk" if value_ok(d, type, 4, False) else "staged"
        out.append(reader + ("-slice" if hi - lo <= MEMBER_SLICE_BITS else "-direct"))
    return out


DENSE_WINDOW = 512   # kDenseWindow
MAPPED_SLICE = 2048  # kMappedSlice


def _reach_form_groups(descs_k, k_type, key_base, key_span, descs_v, v_type, limit, near):
    """dense_plan per segment: the reader ("header", "walk" or "staged"; the walk also asks the value column, when there
    is one, for 1 <= w <= 32, a frame and count * w < 2^31) and, for the other two, "-" + near when the indices the
    segment can reach number at most `limit`, "-direct" otherwise; None for a segment without rows."""
    size, signed = k_type
    sbit = (1 << (8 * size - 1)) if signed else 0
    dlo = (int(key_base) ^ sbit)            # biased by the sign bit every interval is one of unsigned numbers
    dhi = dlo + int(key_span) - 1
    out = []
    for d, dv in zip(descs_k, descs_v if descs_v is not None else repeat(None)):
        if int(d["count"]) == 0:
            out.append(None)
            continue
        m = frame(d, size, signed)
        if m is None:
            out.append("staged-direct")
            continue
        bmin = m + sbit
        btop = bmin + (1 << int(d["width"])) - 1
        if btop < dlo or dhi < bmin:
            out.append("header")
            continue
        lo, hi = max(bmin - dlo, 0), min(btop, dhi) - dlo + 1   # indices [lo, hi) are what the segment can reach
        walk = value_ok(d, k_type, 4, False) and (dv is None or value_ok(dv, v_type, 1, False))
        out.append(("walk" if walk else "staged") + ("-" + near if hi - lo <= limit else "-direct"))
    return out


def dense_form_groups(descs_k, k_type, key_base, key_span, descs_v=None, v_type=None):
    """adac_scan_group_sum_dense (descs_v / v_type given) / adac_scan_group_count_dense: dense_plan, per segment
    "header", "walk-window", "walk-direct", "staged-window" or "staged-direct" (every scan group of a segment takes the
    same form); None for a segment without rows.  member_plan's rule with DENSE_WINDOW indices for the window, the walk
    also asking the value column for 1 <= w <= 32, a frame and count * w < 2^31.  Types: (size in bytes, signed);
    key_base: a bit pattern of the key type."""
    return _reach_form_groups(descs_k, k_type, key_base, key_span, descs_v, v_type, DENSE_WINDOW, "window")


def mapped_form_groups(descs_k, k_type, key_base, key_span, descs_v=None, v_type=None):
    """adac_scan_group_sum_mapped / adac_scan_build_map (descs_v / v_type: the value or the codes column) /
    adac_scan_group_count_mapped: mapped_plan (csrc/adac_group_mapped.inl), per segment "header", "walk-slice",
    "walk-direct", "staged-slice" or "staged-direct"; None for a segment without rows.  dense_form_groups' rule with
    MAPPED_SLICE indices for the on-chip copy of the map (the build has no such copy: only its reader matters)."""
    return _reach_form_groups(descs_k, k_type, key_base, key_span, descs_v, v_type, MAPPED_SLICE, "slice")


def mapped_product_form_groups(descs_k, k_type, key_base, key_span, descs_a, a_type, descs_b, b_type):
    """adac_scan_group_sum_product_mapped: mapped_product_plan (csrc/adac_group_mapped_product.inl), per segment the five
    names of mapped_form_groups.  The key side, the header and the slice are that function's; the walk needs BOTH a and b
    at 1 <= w <= 32 with a frame and count * w < 2^31, and either of them can send the segment to the staged reader."""
    out = []
    for f, da, db in zip(mapped_form_groups(descs_k, k_type, key_base, key_span), descs_a, descs_b):
        if f is not None and f.startswith("walk") and not (value_ok(da, a_type, 1, False) and value_ok(db, b_type, 1, False)):
            f = "staged" + f[len("walk"):]
        out.append(f)
    return out
