"""adac_scan_group_sum_product3 exists in every layer a caller meets — header, library, ctypes table, Layout, tuning
knob — and its kernels, masked and unmasked, are held to their resource limits.  No GPU needed.

The grouped and product kernels that were there before it (k_group_sum*, k_scan_product*, k_group_product<*>,
k_group_product_rw<*>) keep the budget entries they had.  The numpy reference of the GPU tests is checked against Python
integers here."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW = ("k_group_product3<", "k_group_product3_rw<")


def _entry(vgprs, lds, occupancy, sgpr_spills):
    return {"agprs": 0, "lds": lds, "occupancy": occupancy, "scratch": 0, "sgpr_spills": sgpr_spills, "vgpr_spills": 0,
            "vgprs": vgprs}


# profiles/kernel_budget.json before adac_scan_group_sum_product3 was added
BEFORE = {
    "k_group_sum<false>": _entry(52, 20608, 7, 54),
    "k_group_sum<true>": _entry(70, 22688, 7, 67),
    "k_group_sum_rw<false>": _entry(72, 13056, 7, 22),
    "k_group_sum_rw<true>": _entry(80, 13056, 6, 22),
    "k_scan_product<false>": _entry(133, 14464, 3, 0),
    "k_scan_product<true>": _entry(138, 14464, 3, 0),
    "k_group_product<false>": _entry(66, 27840, 5, 184),
    "k_group_product<true>": _entry(87, 29920, 5, 298),
    "k_group_product_rw<false,false>": _entry(101, 22144, 4, 10),
    "k_group_product_rw<false,true>": _entry(104, 26240, 4, 10),
    "k_group_product_rw<true,false>": _entry(108, 22144, 4, 17),
    "k_group_product_rw<true,true>": _entry(109, 26240, 4, 17),
}


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    m = re.search(r"adac_status\s+adac_scan_group_sum_product3\s*\(([^)]*)\)\s*;", text)
    assert m, "include/adacodec.h does not declare adac_scan_group_sum_product3"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 12
    assert "adac_layout" in params[4] and "d_c_words" in params[5] and "keys" in params[6]
    assert "d_validity" in params[8] and "ngroups" in params[9] and "uint32_t" in params[9]
    assert "d_sums" in params[10] and "d_counts" in params[11]
    assert '"group_product3_rw"' in text  # the knob list
    handover = text[text.index("Diagnostic, not part of the drop-in boundary: *left"):]
    assert "adac_scan_group_sum_product3" in handover[:handover.index("adac_debug_group_handover(")]


def test_library_exports_the_entry_point(adac):
    lib = ctypes.CDLL(adac.build())
    assert hasattr(lib, "adac_scan_group_sum_product3")
    assert adac.lib().adac_abi_version() == 1  # an added entry point is compatible


def test_signature_has_twelve_arguments(adac):
    res, args = adac.SIGNATURES["adac_scan_group_sum_product3"]
    assert res is ctypes.c_int and len(args) == 12
    assert args[9] is ctypes.c_uint32
    assert all(ctypes.sizeof(a) == ctypes.sizeof(ctypes.c_void_p) for i, a in enumerate(args) if i != 9)


def test_layout_has_the_method(adac):
    assert callable(getattr(adac.Layout, "scan_group_sum_product3"))


def test_the_knob_is_known(adac):
    adac.build()
    try:
        assert adac.lib().adac_set_tuning(b"group_product3_rw", 0) == 0
    finally:
        assert adac.lib().adac_set_tuning(b"group_product3_rw", 1) == 0


@pytest.fixture(scope="module")
def budgeted(adac):
    import kernel_resources as kr
    adac.build()
    return kr.budgeted(kr.parse())


def test_product3_kernels_are_budgeted_masked_and_unmasked(budgeted):
    mine = {k: v for k, v in budgeted.items() if k.startswith(NEW)}
    for form in NEW:
        names = [k for k in mine if k.startswith(form)]
        assert any("<true" in k for k in names) and any("<false" in k for k in names), sorted(mine)
    assert len(mine) == 6, sorted(mine)  # <V> and <V, C>
    for name, r in mine.items():
        assert r["vgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
    committed = json.load(open(os.path.join(ROOT, "profiles", "kernel_budget.json")))["kernels"]
    assert set(mine) <= set(committed), sorted(set(mine) - set(committed))
    for name in mine:
        assert committed[name]["vgpr_spills"] == 0 and committed[name]["scratch"] == 0, name


def test_the_kernels_that_were_there_keep_their_budget():
    committed = json.load(open(os.path.join(ROOT, "profiles", "kernel_budget.json")))["kernels"]
    assert any(k.startswith(NEW) for k in committed)
    theirs = {k: v for k, v in committed.items()
              if k.startswith(("k_group_sum", "k_scan_product", "k_group_product")) and not k.startswith(NEW)}
    assert theirs == BEFORE


def test_the_numpy_reference_is_the_product_mod_2_64():
    """product3 of tests/test_gpu_group_sum_product3.py — the uint64 product of the three widened columns — equals
    Python integers taken mod 2^64, signed types included"""
    from test_gpu_group_sum_product3 import product3
    rng = np.random.default_rng(3)
    n = 1000
    types = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
    for i in range(len(types)):
        ta, tb, tc = (np.dtype(types[(i + s) % len(types)]) for s in (0, 3, 5))
        cols = []
        for t in (ta, tb, tc):
            info = np.iinfo(t)
            v = rng.integers(info.min, info.max, size=n, dtype=t, endpoint=True)
            v[:4] = [info.min, info.max, info.min, info.max]
            cols.append(v)
        a, b, c = cols
        got = product3(a, b, c)
        assert got.dtype == np.uint64
        want = [(int(x) * int(y) * int(z)) % 2 ** 64 for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())]
        assert got.tolist() == want, (ta.name, tb.name, tc.name)
        assert int(got.sum(dtype=np.uint64)) == sum(want) % 2 ** 64
