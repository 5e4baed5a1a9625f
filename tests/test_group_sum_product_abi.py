"""adac_scan_group_sum_product exists in every layer a caller meets — header, library, ctypes table, Layout, tuning
knob — and its kernels, masked and unmasked, are held to their resource limits.  No GPU needed.

The kernels this scan was composed from (k_group_sum*, k_scan_product*) keep the budget entries they had before it."""
import ctypes
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# profiles/kernel_budget.json before adac_scan_group_sum_product was added
BEFORE = {
    "k_group_sum<false>": {"agprs": 0, "lds": 20608, "occupancy": 7, "scratch": 0, "sgpr_spills": 54, "vgpr_spills": 0,
                           "vgprs": 52},
    "k_group_sum<true>": {"agprs": 0, "lds": 22688, "occupancy": 7, "scratch": 0, "sgpr_spills": 67, "vgpr_spills": 0,
                          "vgprs": 70},
    "k_group_sum_rw<false>": {"agprs": 0, "lds": 13056, "occupancy": 7, "scratch": 0, "sgpr_spills": 22,
                              "vgpr_spills": 0, "vgprs": 72},
    "k_group_sum_rw<true>": {"agprs": 0, "lds": 13056, "occupancy": 6, "scratch": 0, "sgpr_spills": 22,
                             "vgpr_spills": 0, "vgprs": 80},
    "k_scan_product<false>": {"agprs": 0, "lds": 14464, "occupancy": 3, "scratch": 0, "sgpr_spills": 0,
                              "vgpr_spills": 0, "vgprs": 133},
    "k_scan_product<true>": {"agprs": 0, "lds": 14464, "occupancy": 3, "scratch": 0, "sgpr_spills": 0,
                             "vgpr_spills": 0, "vgprs": 138},
}


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    m = re.search(r"adac_status\s+adac_scan_group_sum_product\s*\(([^)]*)\)\s*;", text)
    assert m, "include/adacodec.h does not declare adac_scan_group_sum_product"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 10
    assert "d_validity" in params[6] and "ngroups" in params[7] and "uint32_t" in params[7]
    assert "d_sums" in params[8] and "d_counts" in params[9]
    assert '"group_product_rw"' in text  # the knob list


def test_library_exports_the_entry_point(adac):
    lib = ctypes.CDLL(adac.build())
    assert hasattr(lib, "adac_scan_group_sum_product")
    assert adac.lib().adac_abi_version() == 1  # an added entry point is compatible


def test_signature_has_ten_arguments(adac):
    res, args = adac.SIGNATURES["adac_scan_group_sum_product"]
    assert res is ctypes.c_int and len(args) == 10
    assert args[7] is ctypes.c_uint32
    assert all(ctypes.sizeof(a) == ctypes.sizeof(ctypes.c_void_p) for i, a in enumerate(args) if i != 7)


def test_layout_has_the_method(adac):
    assert callable(getattr(adac.Layout, "scan_group_sum_product"))


def test_the_hand_over_diagnostic_exists(adac):
    text = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    assert re.search(r"adac_status\s+adac_debug_group_handover\s*\(\s*adac_layout\s*\*\w+\s*,\s*uint64_t\s*\*\w+\s*\)\s*;", text)
    assert hasattr(ctypes.CDLL(adac.build()), "adac_debug_group_handover")
    assert len(adac.SIGNATURES["adac_debug_group_handover"][1]) == 2
    assert callable(getattr(adac.Layout, "debug_group_handover"))


def test_the_knob_is_known(adac):
    adac.build()
    try:
        assert adac.lib().adac_set_tuning(b"group_product_rw", 0) == 0
    finally:
        assert adac.lib().adac_set_tuning(b"group_product_rw", 1) == 0


@pytest.fixture(scope="module")
def budgeted(adac):
    import kernel_resources as kr
    adac.build()
    return kr.budgeted(kr.parse())


def test_product_kernels_are_budgeted_masked_and_unmasked(budgeted):
    mine = {k: v for k, v in budgeted.items() if k.startswith("k_group_product")}
    for form in ("k_group_product<", "k_group_product_rw<"):
        names = [k for k in mine if k.startswith(form)]
        assert any("<true" in k for k in names) and any("<false" in k for k in names), sorted(mine)
    for name, r in mine.items():
        assert r["vgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
    committed = json.load(open(os.path.join(ROOT, "profiles", "kernel_budget.json")))["kernels"]
    assert set(mine) <= set(committed), sorted(set(mine) - set(committed))


def test_the_kernels_it_was_composed_from_keep_their_budget():
    committed = json.load(open(os.path.join(ROOT, "profiles", "kernel_budget.json")))["kernels"]
    theirs = {k: v for k, v in committed.items() if k.startswith(("k_group_sum", "k_scan_product"))}
    assert theirs == BEFORE


@pytest.mark.parametrize("name", ["k_group_sum_rw<false>", "k_group_sum<false>", "k_scan_product<false>"])
def test_the_build_keeps_them_too(budgeted, name):
    r, b = budgeted[name], BEFORE[name]
    assert r["vgprs"] <= b["vgprs"] and r["occupancy"] >= b["occupancy"] and r["lds"] <= b["lds"], (name, r)
    assert r["vgpr_spills"] == 0 and r["scratch"] == 0 and r["sgpr_spills"] <= b["sgpr_spills"], (name, r)
