"""The reference's sqllogictest expectations for its BITPACKING codec (tests/golden/bitpacking_sql_cases.json) answered
from the BITPACKING blocks ALONE: adac_bp_plan_create -> adac_bp_write builds the blocks under every forced mode the
file loops over, and the filters and aggregates come from adac_bp_scan_* — no decode, no succinct layout."""
import numpy as np
import pytest

import bp_sql_cases as sc
from oracle import bitpacking as bp

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
AGG_OPS = ("filter_eq", "sum_min_max", "min_max_avg_count", "avg", "avg_approx", "count_valid")


def pack_validity(valid):
    bits = np.packbits(valid, bitorder="little")
    return np.concatenate([bits, np.zeros((-len(bits)) % 8 + 8, np.uint8)]).view(np.uint64)


@pytest.mark.parametrize("case_id", sc.case_ids())
def test_sql_expectations_from_the_blocks_alone(adac, gpu_ctx, case_id):
    ctx = gpu_ctx
    case = next(c for c in sc.load_cases() if c["id"] == case_id)
    vals, valid = sc.build_column(case)
    dtype, n = vals.dtype, len(vals)
    info = np.iinfo(dtype)
    udtype = np.dtype("u%d" % dtype.itemsize)

    def bits(x):
        return int(np.array([x], dtype=dtype).view(udtype)[0])

    def typed(b):
        return int(np.array([b], dtype=udtype).view(dtype)[0])

    live = vals if valid is None else vals[valid]
    py_sum = sum(int(x) for x in live) & M64
    d_vals = ctx.upload(vals)
    d_valid = None if valid is None else ctx.upload(pack_validity(valid))
    for mode in case["forced_modes"]:
        plan = adac.BitpackingPlan(ctx, dtype, d_vals, n, d_valid, sc.MODE_CODE[mode])
        if sc.refused(case):
            assert not plan.encodable, (case_id, mode)
            continue
        if case.get("may_be_refused") and not plan.encodable:
            with pytest.raises(ValueError):
                bp.Compressed(vals, valid, force_mode=sc.MODE_CODE[mode])
            continue
        assert plan.encodable, (case_id, mode)
        nseg = plan.nseg
        d_blocks = ctx.alloc(max(nseg, 1) * plan.BLOCK_STRIDE + 64)
        plan.write(d_vals, d_blocks, d_valid)
        counts = np.array([plan.segment(i)[1] for i in range(nseg)], dtype=np.uint32)
        lay = adac.BitpackingLayout(ctx, dtype, np.arange(nseg, dtype=np.uint64) * np.uint64(plan.BLOCK_STRIDE), counts)
        assert lay.value_span == n
        nwords = (n + 63) // 64

        def fresh(words):
            return ctx.alloc(words * 8 + 8).upload(np.full(words * 8 + 8, 0xA5, dtype=np.uint8))

        def aggregates(d_mask):  # (sum mod 2^64, min, max, count) of the rows under the mask
            d_sum, d_mm, d_cnt = fresh(nseg), fresh(2 * nseg), fresh(nseg)
            lay.scan_sum(d_blocks, d_sum, d_mask)
            lay.scan_min_max(d_blocks, d_mm, d_mask)
            lay.scan_count_between(d_blocks, bits(info.min), bits(info.max), d_cnt, d_mask)
            mm = d_mm.download(np.uint64, 2 * nseg)
            count = int(d_cnt.download(np.uint64, nseg).sum())
            total = int(d_sum.download(np.uint64, nseg).sum(dtype=np.uint64))
            if count == 0:
                return total, None, None, 0
            segs = [i for i in range(nseg) if typed(mm[2 * i]) <= typed(mm[2 * i + 1])]
            return total, min(typed(mm[2 * i]) for i in segs), max(typed(mm[2 * i + 1]) for i in segs), count

        whole = aggregates(d_valid)
        assert whole[3] == len(live) and whole[0] == py_sum, (case_id, mode, whole)
        for e in case["expect"]:
            op = e["op"]
            if op not in AGG_OPS:
                continue
            if op == "filter_eq":
                d_bm, d_cnt = fresh(nwords), fresh(nseg)
                lay.scan_select_between(d_blocks, bits(e["key"]), bits(e["key"]), d_bm, d_cnt, d_valid)
                got = aggregates(d_bm)
                assert int(d_cnt.download(np.uint64, nseg).sum()) == got[3]
                assert got == (e["sum"] & M64, e["min"], e["max"], e["count"]), (e, got, mode)
            elif op == "sum_min_max":
                assert whole[:3] == (e["sum"] & M64, e["min"], e["max"]), (e, whole, mode)
            elif op == "min_max_avg_count":
                assert whole[1:] == (e["min"], e["max"], e["count"]), (e, whole, mode)
                avg = sum(int(x) for x in live) / len(live)
                assert abs(avg - e["avg"]) <= 1e-9 * max(1.0, abs(e["avg"])), e
            elif op == "count_valid":
                assert whole[3] == e["count"], (e, whole, mode)
            else:  # avg / avg_approx: the device sum mod 2^64 is the Python-int sum of the valid rows mod 2^64
                avg = sum(int(x) for x in live) / whole[3]
                if op == "avg":
                    assert avg == e["value"], e
                else:
                    assert abs(avg - e["value"]) <= e["rel"] * abs(e["value"]), e
