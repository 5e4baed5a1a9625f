"""The oracle against the hand-pinned BITPACKING decision table (tests/bp_decision_cases.py): mode and width of
every group, refusals, the block placement rule at an exactly full block and one byte short, and the width sweeps
the device tests run.  CPU only."""
import numpy as np
import pytest

import bp_decision_cases as T
from oracle import bitpacking as bp


def oracle_groups(comp):
    out = []
    for i in range(comp.nseg):
        for g in range((comp.count(i) + T.GROUP - 1) // T.GROUP):
            mode, _, w = comp.group_info(i, g)
            out.append((mode, w))
    return out


def compress(values, valid, force):
    try:
        return bp.Compressed(values, valid, force, null_zero=valid is not None)
    except ValueError:
        return None


@pytest.mark.parametrize("case", T.CASES, ids=[c.id for c in T.CASES])
def test_decision_table(case):
    comp = compress(case.values, case.valid, case.force)
    if case.expect is T.REFUSED:
        assert comp is None, (case.id, case.cite, oracle_groups(comp))
        return
    assert comp is not None, (case.id, case.cite)
    assert oracle_groups(comp) == case.expect, case.cite
    got = np.concatenate([comp.scan(i) for i in range(comp.nseg)])
    ok = np.ones(len(got), bool) if case.valid is None else case.valid
    assert np.array_equal(got[ok], case.values[ok])
    if case.valid is not None:   # without null_zero the NULL slots keep stale buffer content; valid rows do not care
        stale = bp.Compressed(case.values, case.valid, case.force)
        assert oracle_groups(stale) == case.expect
        got = np.concatenate([stale.scan(i) for i in range(stale.nseg)])
        assert np.array_equal(got[ok], case.values[ok])


def test_table_covers_the_issue_edges():
    names = {}
    for c in T.CASES:
        names.setdefault(c.name, set()).add(c.dtype.name)
    for n in ("for_span_ts_max", "for_span_ts_max_plus_1", "delta_offset_overflows", "delta_range_overflows",
              "one_delta_overflows"):
        assert {"int8", "int16", "int32", "int64"} <= names[n], n
    for n in ("unsigned_max_at_ts_max", "unsigned_max_above_ts_max"):
        assert names[n] == {"uint8", "uint16", "uint32", "uint64"}, n
    for n in ("descending_delta_for", "constant_delta_negative_step", "all_null_group", "null_at_row_0",
              "null_at_row_1", "tail_1_row", "tail_2_rows", "rows_2047"):
        assert len(names[n]) == 8, n
    i64 = [c for c in T.CASES if c.name == "for_overflow_narrow_deltas" and c.dtype == np.int64]
    assert {c.force: c.expect for c in i64} == {T.AUTO: [T.DF(20)], T.CONSTANT: [T.DF(20)],
                                                T.CONSTANT_DELTA: [T.DF(20)], T.DELTA_FOR: [T.DF(20)],
                                                T.FOR: T.REFUSED}
    assert all(c.expect is T.REFUSED for c in T.CASES
               if c.name == "for_overflow_narrow_deltas" and c.dtype != np.int64)
    assert all(c.cite for c in T.CASES)


@pytest.mark.parametrize("dtype,short", T.FILL_SHAPES, ids=["%s-%d" % (np.dtype(d).name, s) for d, s in T.FILL_SHAPES])
def test_block_fill_boundary(dtype, short):
    v, groups, b = T.fill_shape(dtype, short)
    segs, slack = T.place(dtype, groups)
    # the shape really occurs: the boundary group leaves exactly 0 bytes, or misses by `short` bytes
    assert slack[b] == -short
    assert all(s >= 0 for s in slack[:b])
    assert len(segs) == 2 and segs[0][1] == (b + (short == 0)) * T.GROUP
    comp = bp.Compressed(v)
    assert oracle_groups(comp) == [(m, w) for _, m, w in groups]
    assert [(comp.start(i), comp.count(i), comp.size(i)) for i in range(comp.nseg)] == segs
    assert np.array_equal(np.concatenate([comp.scan(i) for i in range(comp.nseg)]), v)


@pytest.mark.parametrize("dtype", T.ALL, ids=[np.dtype(d).name for d in T.ALL])
def test_width_sweeps(dtype):
    v, exp = T.for_sweep(dtype)
    comp = bp.Compressed(v, force_mode=T.FOR)
    assert oracle_groups(comp) == exp
    assert np.array_equal(np.concatenate([comp.scan(i) for i in range(comp.nseg)]), v)
    bits = 8 * np.dtype(dtype).itemsize
    ts = np.dtype(dtype).itemsize
    # every width up to the GetEffectiveWidth jump, and B itself (int8 spans stop at 127: 7 bits, kept at 7)
    assert {w for _, w in exp} == set(range(bits - ts + 1)) | (set() if np.dtype(dtype) == np.int8 else {bits})
    for desc in (False, True):
        v, exp = T.delta_for_sweep(dtype, desc)
        comp = bp.Compressed(v, force_mode=T.DELTA_FOR)
        assert oracle_groups(comp) == exp, desc
        assert np.array_equal(np.concatenate([comp.scan(i) for i in range(comp.nseg)]), v)
        assert sorted(w for m, w in exp if m == T.DELTA_FOR) == list(range(T.max_delta_width(dtype) + 1))
