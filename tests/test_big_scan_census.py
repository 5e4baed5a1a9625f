"""What tests/test_gpu_big_segment_scans.py relies on, stated on the CPU (nothing is launched).

For every cell of big_scan_cases.CELLS the descriptors an encode must produce are built from numpy's min / max and the
reference's width rule, and forms.py must then name the forms the cell claims: the segment below 2^31 bits on the
register walk ("fast" / "walk-*"), the segment at the gate on the staged reader ("generic" / "staged-*"), also when the
big column is only a partner; no compare cell decided by the headers; the narrow domains on the slice / window and
k16's full domain on the direct access.  Plus what the cells assume of their columns and masks."""
import numpy as np
import pytest

import big_scan_cases as cases
from big_scan_cases import BIG, K16_FULL, K16_SLICE, K16_WINDOW
from test_gpu_big_segments import B31, B32, mask_words, rows_below, rows_reaching, threshold_rows


def test_the_matrix_is_complete():
    """every family has its cells; every cell has the big column in exactly one role"""
    want = {"group_sum_valid": {"u32-value"},
            "group_sum_product": {"u32-a", "u32-a-masked", "u32-b", "u32-b-masked", "u64-a", "u64-a-masked"},
            "group_sum_product3": {"u32-c"}, "group_sum_q1": {"u32-q", "u32-a"},
            "compare": {"u32-a", "u32-b", "u64-a", "u8-a"},
            "member": {"k16-select-count", "k16-select-count-masked", "k16-build", "u8-select-count",
                       "u8-select-count-masked"},
            "dense": {"k16-key-full", "k16-key-window", "u32-value", "u64-value"},
            "mapped": {"k16-key-full-build", "k16-key-full", "k16-key-slice"},
            "product_mapped": {"k16-key-full", "u32-a", "u32-b", "u64-a"}}
    assert set(want) == set(cases.FAMILIES)
    for family in cases.FAMILIES:
        cells = cases.cells_of(family)
        assert {x.id for x in cells} == want[family] and len(cells) == len(want[family])
        for x in cells:
            assert [m for _, m in x.roles].count(BIG) == 1 and x.column in cases.BIG_COLUMNS
            assert (x.knob in cases.RW_KNOBS) == family.startswith("group_sum")
    assert K16_WINDOW[0] >= K16_SLICE[0] and sum(K16_WINDOW) <= sum(K16_SLICE)     # the slice holds the window


@pytest.mark.parametrize("name", cases.BIG_COLUMNS)
def test_cells_are_what_they_claim(oracle, name):
    c = cases.big_column(name)
    width_of = oracle.width_from_succinct
    big = cases.expected_descs(width_of, c.vals, c.counts)
    assert [d["width"] for d in big] == c.widths and [d["min"] for d in big] == [mn for mn, _ in c.minmax]
    bits = [d["count"] * d["width"] for d in big]
    cache, made = {}, {}
    for cell in cases.cells_of(column=name):
        vals = cell.partner_values(c, cache)
        descs, kinds = {}, {}
        for role, maker in cell.roles:
            if maker not in made:
                made[maker] = big if maker is BIG else cases.expected_descs(width_of, vals[role], c.counts)
            descs[role], kinds[role] = made[maker], cases.kind(vals[role].dtype)
            if maker is not BIG:
                # a partner never reaches a gate itself: where a segment is sent to the staged form, the big column did it
                assert all(d["count"] * d["width"] < B31 for d in descs[role]) or maker == "twin", (cell.id, role)
                assert role not in ("a", "key") or all(d["width"] >= 4 for d in descs[role]), (cell.id, role)
        cell.check_forms(descs, kinds, "census")
        if cell.family == "compare":
            assert "header" not in cell.forms(descs, kinds)
            lt, eq, _ = cases.sc.compare_masks(vals["a"], vals["b"])
            for s in c.big:
                seg = slice(c.offs[s], c.offs[s] + int(c.counts[s]))
                assert np.count_nonzero(eq[seg]) > 0 and 0.05 < lt[seg].mean() < 0.95, (cell.id, s)
            del lt, eq
        if cell.mask is not None:
            keep = mask_words(c.n, cell.mask)[1]
            assert any(o % 64 for o in c.offs[1:])                       # a segment starts inside a mask word
            for s in c.big:
                for r in threshold_rows(int(c.counts[s]), c.widths[s]):
                    e = c.offs[s] + r
                    for side in (keep[max(0, e - 32):e], keep[e + 1:e + 33]):
                        assert len(side) == 0 or (side.any() and not side.all()), (cell.id, s, r)
    if name == "u32":
        assert bits[0] < B31 <= bits[1]
    elif name == "u64":
        assert bits[0] >= B32 and bits[1] >= B32
    elif name == "u8":
        assert bits[0] >= B31 and int(c.counts[0]) // 32 > 1 << 23
    else:
        assert rows_below(B31, 15) == 143_165_576 and rows_reaching(B31, 15) == 143_165_577
        assert c.counts.tolist() == [143_165_576, 143_165_577, 4097]
        assert bits[0] < B31 <= bits[1] and bits[0] + 15 >= B31 > bits[1] - 15    # the nearest counts on either side
        planted = cases.planted_rows(c)
        assert {s for _, s in planted} == {0, 1} and len(planted) >= 3
        assert {e - c.offs[s] for e, s in planted} >= {int(c.counts[0]) - 1, int(c.counts[1]) - 2, int(c.counts[1]) - 1}
        for base, span in (K16_WINDOW, K16_SLICE, K16_FULL):
            assert all(base <= int(c.vals[e]) < base + span for e, _ in planted)
            assert base <= int(c.segs[2][-1]) < base + span             # the small segment's last row, as it is
        # every key of the full domain occurs in both big segments: the built set is full, the built map has no fill
        for s in c.big:
            assert np.bincount(c.segs[s], minlength=K16_FULL[0] + K16_FULL[1])[K16_FULL[0]:].min() > 0
        inside = (c.vals >= K16_WINDOW[0]) & (c.vals < sum(K16_WINDOW))
        assert all(0.005 < inside[o:o + int(n)].mean() < 0.9 for o, n in zip(c.offs, c.counts))   # rows in and out
        assert 0 < int(cases.sparse_keep(c).sum()) < c.n // 1000
