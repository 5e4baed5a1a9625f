"""Seeded differential fuzz of the device BITPACKING compress against the oracle, with a generator that reaches
the decision edges of BitpackingState::Flush: values anywhere in T's range (above NumericLimits<T_S>::Maximum() for
unsigned types, next to MIN / MAX for signed ones), descending runs and negative steps, spans up to the full width
and exactly T_S's maximum, NULL masks with all-NULL groups, lengths 1, 2, 2047-2049 and multi-block columns, and a
forced mode on about a fifth of the seeds.  tools/soak_bitpacking.py runs the same generator over many more seeds."""
import numpy as np
import pytest

from bp_decision_cases import lim
from oracle import bitpacking as bp
from test_gpu_bitpacking import assert_blocks_equal_oracle, gpu_compress
from test_gpu_bitpacking_decisions import check_decode

pytestmark = pytest.mark.gpu
ALL = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
M64 = (1 << 64) - 1


def _u(x):
    return np.uint64(int(x) & M64)


def _rand_int(rng, lo, hi):
    """uniform in [lo, hi] for Python ints spanning up to 2^64 values"""
    return lo + int(rng.integers(0, hi - lo, endpoint=True, dtype=np.uint64))


def _part(rng, dtype, m, kind):
    """m values of one pattern, as uint64 bit patterns (two's complement; narrower types keep the low bits)"""
    bits, ms, tmin, tmax = lim(dtype)
    sg = np.dtype(dtype).kind == "i"
    idx = np.arange(m, dtype=np.uint64)
    edge = [tmin, tmax, tmin + 1, tmax - 1, ms, ms + 1 if not sg else -1, 0]
    if kind == 0:                                   # constant, often at an edge
        x = edge[int(rng.integers(0, len(edge)))] if rng.random() < 0.5 else _rand_int(rng, tmin, tmax)
        return np.full(m, _u(x), dtype=np.uint64)
    if kind == 1:                                   # arithmetic run, either sign, may wrap
        step = int(rng.integers(-7, 8)) * (1 if rng.random() < 0.7 else int(rng.integers(1, 1 << (bits - 8) + 1)))
        total = step * (m - 1)
        if rng.random() < 0.3 or not tmin <= tmin - min(total, 0) <= tmax - max(total, 0):
            return _u(_rand_int(rng, tmin, tmax)) + _u(step) * idx
        return _u(_rand_int(rng, tmin - min(total, 0), tmax - max(total, 0))) + _u(step) * idx
    if kind == 2:                                   # sorted run, ascending or descending, mostly within range
        kk = int(rng.integers(0, min(bits - 2, 24) + 1))
        if rng.random() < 0.7:
            kk = min(kk, max(0, bits - 13))
        c = np.cumsum(rng.integers(0, 1 << kk, size=m, dtype=np.uint64), dtype=np.uint64)
        total = int(c[-1])
        desc = rng.random() < 0.5
        if rng.random() < 0.7 and total <= tmax - tmin:
            v0 = _rand_int(rng, tmin + total, tmax) if desc else _rand_int(rng, tmin, tmax - total)
        else:
            v0 = _rand_int(rng, tmin, tmax)
        return _u(v0) - c if desc else _u(v0) + c
    if kind == 3:                                   # random span of w bits anywhere in range, w up to B
        w = int(rng.integers(0, bits + 1))
        span = min((1 << w) - 1, tmax - tmin)
        lo = _rand_int(rng, tmin, tmax - span)
        v = _u(lo) + rng.integers(0, span, endpoint=True, size=m, dtype=np.uint64)
        if m > 2:
            v[0], v[m - 1] = _u(lo), _u(lo + span)
        return v
    if kind == 4:                                   # next to MIN / MAX
        r = int(rng.integers(0, bits))
        off = rng.integers(0, 1 << r, size=m, dtype=np.uint64)
        return _u(tmin) + off if rng.random() < 0.5 else _u(tmax) - off
    if kind == 5:                                   # unsigned: straddle T_S max; signed: span exactly T_S max
        if not sg:
            d = int(rng.integers(0, 200))
            return _u(ms - d) + (idx if rng.random() < 0.5 else rng.integers(0, 2 * d + 2, size=m, dtype=np.uint64))
        lo = _rand_int(rng, tmin, tmax - ms)
        v = _u(lo) + rng.integers(0, ms, endpoint=True, size=m, dtype=np.uint64)
        if m > 2:
            v[1], v[m - 1] = _u(lo), _u(lo + ms)
        return v
    if kind == 6:                                   # a ramp whose span crosses T_S max with narrow deltas
        step = ((tmax - tmin) // max(m, 1)) * int(rng.integers(5, 10)) // 10
        kk = int(rng.integers(0, 6))
        c = np.cumsum(rng.integers(0, 1 << kk, size=m, dtype=np.uint64), dtype=np.uint64)
        return _u(tmin + int(rng.integers(0, 1 << 8))) + _u(step) * idx + c
    return rng.integers(0, (1 << bits) - 1, endpoint=True, size=m, dtype=np.uint64)   # whole range


def random_column(rng):
    """(values, validity or None, force mode)"""
    dtype = np.dtype(ALL[int(rng.integers(0, len(ALL)))])
    ts = dtype.itemsize
    multi = rng.random() < 0.06
    if multi:   # wide random groups over more than two 256 KiB blocks
        n = int(2.3 * 262144 / ts) + int(rng.integers(0, 5000))
    else:
        n = int(rng.choice([1, 2, 3, 2047, 2048, 2049, 4095, 4097, int(rng.integers(1, 9000)),
                            int(rng.integers(9000, 30000))]))
    parts, left = [], n
    while left > 0:
        m = min(left, int(rng.choice([2048, 2048, 4096, int(rng.integers(1, 5000))])))
        kind = 7 if multi else int(rng.integers(0, 8))
        parts.append(_part(rng, dtype, m, kind))
        left -= m
    v = np.concatenate(parts)[:n].astype(np.dtype("u%d" % ts)).view(dtype)
    valid = None
    if rng.random() < 0.3:
        valid = rng.random(n) > rng.random() * 0.7
        if rng.random() < 0.4 and n > 2048:
            g = int(rng.integers(0, (n + 2047) // 2048))
            valid[g * 2048:(g + 1) * 2048] = False
    force = int(rng.integers(1, 5)) if rng.random() < 0.2 else 0
    return v, valid, force


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
