"""The scan families that came after test_gpu_big_segments.py, each on one segment just below and one at or past 2^31 /
2^32 bits: where its width-templated register walk hands over to its staged reader, and where that reader mixes 64-bit
bit positions with 32-bit row, chunk and dword arithmetic.

One test function per family, one case per cell of big_scan_cases.CELLS ("u32-a": the big u32 column in role a, its
partners narrow).  Every case encodes its partners, states the forms of every segment on the DEVICE's descriptors with
forms.py (the statements test_big_scan_census.py makes on the CPU), runs the entry points into outputs poisoned with
0xEE bytes whose spare word must keep the poison, compares every word with numpy over the raw values (no tolerance)
and frees its partners.  The four families with a register-walk knob run with the knob at 1, 0 and 1 again and hold
adac_debug_group_handover against forms.py each time; the last test holds that every knob is back at its default.

The columns are test_gpu_big_segments.py's u32, u64 and u8 and the dense key column k16 of big_scan_cases.py."""
import numpy as np
import pytest

import big_scan_cases as cases
from test_gpu_big_segments import column, encoded  # noqa: F401  (the module-scoped fixture of the encoded big column)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k16(adac, gpu_ctx):
    yield from encoded(adac, gpu_ctx, cases.make_k16())


def on_u32_u64_u8(family):
    """one case per cell of the family on a column of test_gpu_big_segments.py, selected through its `column` fixture"""
    params = [pytest.param(x.column, x, id=x.id) for x in cases.cells_of(family) if x.column != "k16"]
    return pytest.mark.parametrize("column,cell", params, indirect=["column"])


def on_k16(family):
    """one case per cell of the family on the dense key column, which has a fixture of its own (a family with cells of
    both kinds has a test function for each)"""
    return pytest.mark.parametrize("cell", [pytest.param(x, id=x.id) for x in cases.cells_of(family, "k16")])


@on_u32_u64_u8("group_sum_valid")
def test_group_sum_valid(adac, gpu_ctx, column, cell):
    cases.run_cell(adac, gpu_ctx, column, cell)


@on_u32_u64_u8("group_sum_product")
def test_group_sum_product(adac, gpu_ctx, column, cell):
    cases.run_cell(adac, gpu_ctx, column, cell)


@on_u32_u64_u8("group_sum_product3")
def test_group_sum_product3(adac, gpu_ctx, column, cell):
    cases.run_cell(adac, gpu_ctx, column, cell)


@on_u32_u64_u8("group_sum_q1")
def test_group_sum_q1(adac, gpu_ctx, column, cell):
    cases.run_cell(adac, gpu_ctx, column, cell)


@on_u32_u64_u8("compare")
def test_select_and_count_compare(adac, gpu_ctx, column, cell):
    cases.run_cell(adac, gpu_ctx, column, cell)


@on_u32_u64_u8("member")
def test_member_scans(adac, gpu_ctx, column, cell):
    cases.run_cell(adac, gpu_ctx, column, cell)


@on_k16("member")
def test_member_scans_on_the_dense_key(adac, gpu_ctx, k16, cell):
    cases.run_cell(adac, gpu_ctx, k16, cell)


@on_u32_u64_u8("dense")
def test_group_dense_by_value(adac, gpu_ctx, column, cell):
    cases.run_cell(adac, gpu_ctx, column, cell)


@on_k16("dense")
def test_group_dense_by_key(adac, gpu_ctx, k16, cell):
    cases.run_cell(adac, gpu_ctx, k16, cell)


@on_k16("mapped")
def test_build_map_and_group_mapped(adac, gpu_ctx, k16, cell):
    cases.run_cell(adac, gpu_ctx, k16, cell)


@on_u32_u64_u8("product_mapped")
def test_group_product_mapped_by_value(adac, gpu_ctx, column, cell):
    cases.run_cell(adac, gpu_ctx, column, cell)


@on_k16("product_mapped")
def test_group_product_mapped_by_key(adac, gpu_ctx, k16, cell):
    cases.run_cell(adac, gpu_ctx, k16, cell)


def test_every_cell_has_a_test():
    here = [on_u32_u64_u8(f).args[1] for f in cases.FAMILIES] + [on_k16(f).args[1] for f in cases.FAMILIES]
    assert sum(len(p) for p in here) == len(cases.CELLS)


def test_knobs_are_back_at_their_defaults(adac, gpu_ctx):
    """After the module: every register-walk knob is at 1 again.  A two-segment table whose second segment has a value
    column of w 2 (under the walk's 4 bits): with its knob on, each family's walk is launched and leaves exactly that
    segment's scan groups to the staged kernel; with the knob at 0 the hand-over word would be 0."""
    env = cases.Env(adac, gpu_ctx)
    counts = np.array([5000, 5000], dtype=np.uint32)
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.integers(0, 1 << 10, 5000), rng.integers(0, 4, 5000)]).astype(np.uint32)
    narrow = rng.integers(0, 32, 10000).astype(np.uint16)
    keys = rng.integers(0, cases.NGROUPS, 10000).astype(np.uint8)
    A, N, K = env.encode(a, counts), env.encode(narrow, counts), env.encode(keys, counts)
    assert A.descs["width"].tolist() == [10, 2]
    G = cases.NGROUPS
    outs = [env.out(cases.TERMS * (G + 1)), env.out(G + 1)]
    o, p = outs[0][0], outs[1][0]
    calls = {
        "group_sum_rw": ([A], lambda: A.lay.scan_group_sum_valid(A.words, K.lay, K.words, None, G, o, p)),
        "group_product_rw": ([A, N], lambda: A.lay.scan_group_sum_product(A.words, N.lay, N.words, K.lay, K.words, G, o, p)),
        "group_product3_rw": ([A, N, N], lambda: A.lay.scan_group_sum_product3(A.words, N.lay, N.words, N.lay, N.words,
                                                                             K.lay, K.words, G, o, p)),
        "group_q1_rw": ([A, N, N, N], lambda: A.lay.scan_group_sum_q1(A.words, N.lay, N.words, N.lay, N.words, N.lay,
                                                                      N.words, K.lay, K.words, G, o)),
    }
    assert set(calls) == set(cases.RW_KNOBS)
    for knob, (values, launch) in calls.items():
        left = cases.generic_scan_groups([s.descs for s in values], [s.kind for s in values], K.descs)
        assert left > 0
        env.call(outs, launch)
        assert A.lay.debug_group_handover() == left, knob
    for side in (A, N, K):
        side.free()
    for buf, _ in outs:
        buf.free()
