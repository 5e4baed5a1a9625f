"""Seeded differential fuzz of the device BITPACKING compress against the oracle, with a generator that reaches
the decision edges of BitpackingState::Flush: values anywhere in T's range (above NumericLimits<T_S>::Maximum() for
unsigned types, next to MIN / MAX for signed ones), descending runs and negative steps, spans up to the full width
and exactly T_S's maximum, NULL masks with all-NULL groups, lengths 1, 2, 2047-2049 and multi-block columns, and a
forced mode on about a fifth of the seeds.  tools/soak_bitpacking.py runs the same generator over many more seeds."""
import numpy as np
import pytest

from bp_fuzz_columns import ALL, M64, _part, _rand_int, _u, random_column  # noqa: F401  (tools/soak_bitpacking.py)
from oracle import bitpacking as bp
from test_gpu_bitpacking import assert_blocks_equal_oracle, gpu_compress
from test_gpu_bitpacking_decisions import check_decode

pytestmark = pytest.mark.gpu


def check_seed(adac, ctx, seed):
    rng = np.random.default_rng(seed)
    v, valid, force = random_column(rng)
    try:
        comp = bp.Compressed(v, valid, force, null_zero=valid is not None)
    except ValueError:
        comp = None
    plan, d_blocks, _ = gpu_compress(adac, ctx, v, valid, force)
    assert plan.encodable == (comp is not None), (seed, v.dtype.name, len(v), force)
    if comp is None:
        return False
    assert_blocks_equal_oracle(plan, d_blocks, comp)
    extra = tuple(int(x) for x in rng.integers(0, 2 * 2048, size=3))
    check_decode(adac, ctx, plan, d_blocks, v, valid, starts=(1, 31, 32, 1000, 2047) + extra)
    return True


SEEDS = list(range(150))


@pytest.mark.parametrize("block", range(5))
def test_bitpacking_fuzz(adac, gpu_ctx, block):
    encoded = 0
    for seed in SEEDS[block::5]:
        encoded += check_seed(adac, gpu_ctx, 70_000 + seed)
    assert encoded >= 10   # most columns are encodable; refusals are checked too
