"""adac_scan_sum_product exists in every layer a caller meets — header, library, ctypes table, Layout — and its kernels
are held to the register budget.  No GPU needed."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    m = re.search(r"adac_status\s+adac_scan_sum_product\s*\(([^)]*)\)\s*;", text)
    assert m, "include/adacodec.h does not declare adac_scan_sum_product"
    assert len(m.group(1).split(",")) == 6


def test_library_exports_the_entry_point(adac):
    lib = ctypes.CDLL(adac.build())
    assert hasattr(lib, "adac_scan_sum_product")
    assert adac.lib().adac_abi_version() == 1  # an added entry point is compatible


def test_signature_has_six_pointer_sized_arguments(adac):
    res, args = adac.SIGNATURES["adac_scan_sum_product"]
    assert res is ctypes.c_int
    assert len(args) == 6 and all(ctypes.sizeof(a) == ctypes.sizeof(ctypes.c_void_p) for a in args)


def test_layout_has_the_method(adac):
    assert callable(getattr(adac.Layout, "scan_sum_product"))


def test_product_kernels_are_budgeted_without_spills(adac):
    import kernel_resources as kr
    adac.build()
    mine = {k: v for k, v in kr.budgeted(kr.parse()).items() if k.startswith("k_scan_product")}
    assert mine, "no k_scan_product kernel among the budgeted kernels"
    for name, r in mine.items():
        assert r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
