"""adac_scan_group_sum_dense at device sizes other than the whole device's (tuning knob "num_cus", as in
tests/test_gpu_grid_sizes.py): the kernel takes one workgroup per scan group whatever the knob says, so the columns of
test_gpu_group_dense.py's several-groups case must give the same sums at every setting."""
import numpy as np
import pytest

from dense_cases import check_dense, dense_forms
from test_gpu_group_dense import GROUP_CASES, two_group_column
from test_gpu_sum_product import encode_column

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("num_cus", [1, 3, 64])
def test_two_scan_groups_at_other_device_sizes(adac, gpu_ctx, num_cus):
    dtype, w, span, want = GROUP_CASES[1]   # walk-direct
    keys, vals, base = two_group_column(dtype, w, span, want)
    counts = np.array([len(keys)], dtype=np.uint32)
    adac.set_tuning("num_cus", num_cus)
    try:
        klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
        vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
        assert dense_forms(klay, base, span, vlay) == [want]
        _, c, inside = check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span, what=num_cus)
        assert inside[-1] and int(c[span // 2]) >= 2
    finally:
        adac.set_tuning("num_cus", 0)
