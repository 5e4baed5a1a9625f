"""adac_scan_group_sum_valid exists in every layer a caller meets — header, library, ctypes table, Layout — and the
grouped scan's kernels, masked and unmasked, are held to their register budget.  No GPU needed.

The bounds on the two unmasked kernels are the entries profiles/kernel_budget.json held for `k_group_sum_rw` and
`k_group_sum` before the kernels became templates on the mask: taking a mask must not cost the unmasked call anything."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    m = re.search(r"adac_status\s+adac_scan_group_sum_valid\s*\(([^)]*)\)\s*;", text)
    assert m, "include/adacodec.h does not declare adac_scan_group_sum_valid"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 8
    assert "d_validity" in params[4] and "ngroups" in params[5]
    assert re.search(r"adac_status\s+adac_scan_group_sum\s*\(", text)  # the unmasked call stays


def test_library_exports_the_entry_point(adac):
    lib = ctypes.CDLL(adac.build())
    assert hasattr(lib, "adac_scan_group_sum_valid") and hasattr(lib, "adac_scan_group_sum")
    assert adac.lib().adac_abi_version() == 1  # an added entry point is compatible


def test_signature_has_eight_arguments(adac):
    res, args = adac.SIGNATURES["adac_scan_group_sum_valid"]
    assert res is ctypes.c_int and len(args) == 8
    assert args[5] is ctypes.c_uint32
    assert all(ctypes.sizeof(a) == ctypes.sizeof(ctypes.c_void_p) for i, a in enumerate(args) if i != 5)
    assert adac.SIGNATURES["adac_scan_group_sum"][1] == args[:4] + args[5:]


def test_layout_has_the_method(adac):
    assert callable(getattr(adac.Layout, "scan_group_sum_valid"))
    assert callable(getattr(adac.Layout, "scan_group_sum"))


@pytest.fixture(scope="module")
def group_kernels(adac):
    import kernel_resources as kr
    adac.build()
    return {k: v for k, v in kr.budgeted(kr.parse()).items() if k.startswith("k_group_sum")}


def test_group_sum_kernels_do_not_spill_vgprs(group_kernels):
    assert group_kernels, "no k_group_sum kernel among the budgeted kernels"
    for name, r in group_kernels.items():
        assert r["vgpr_spills"] == 0 and r["scratch"] == 0, (name, r)


def test_both_kernels_have_a_masked_instantiation(group_kernels):
    assert "k_group_sum_rw<true>" in group_kernels and "k_group_sum<true>" in group_kernels, sorted(group_kernels)
    assert "k_group_sum_rw<false>" in group_kernels and "k_group_sum<false>" in group_kernels, sorted(group_kernels)


@pytest.mark.parametrize("name,vgprs,lds,sgpr_spills", [("k_group_sum_rw<false>", 72, 13056, 22),
                                                       ("k_group_sum<false>", 52, 20608, 54)])
def test_unmasked_kernels_stay_within_their_old_budget(group_kernels, name, vgprs, lds, sgpr_spills):
    r = group_kernels[name]
    assert r["vgprs"] <= vgprs and r["occupancy"] >= 7 and r["lds"] <= lds, (name, r)
    assert r["vgpr_spills"] == 0 and r["scratch"] == 0 and r["sgpr_spills"] <= sgpr_spills, (name, r)
