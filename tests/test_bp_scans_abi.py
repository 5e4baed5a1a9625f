"""The fused scans on BITPACKING blocks as an interface (no GPU): the header declares them, the library exports them,
the Python binding carries them, and the compiler's resource remarks show the new kernels free of spills and scratch."""
import ctypes as C
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"adac_bp_layout_value_span": 1, "adac_bp_scan_sum": 4, "adac_bp_scan_count_between": 6,
        "adac_bp_scan_select_between": 7, "adac_bp_scan_min_max": 4}


@pytest.fixture(scope="module")
def lib(adac):
    adac.build()
    return adac.lib()


def test_header_declares_the_five_entry_points():
    hdr = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "#define ADAC_ABI_VERSION 1" in hdr
    for name, nargs in ARGS.items():
        m = re.search(r"\b(adac_status|uint64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        assert len(m.group(2).split(",")) == nargs, (name, m.group(2))
        assert (m.group(1) == "uint64_t") == (name == "adac_bp_layout_value_span")


def test_library_exports_and_binding_holds_them(adac, lib):
    raw = C.CDLL(adac.LIB_PATH)
    for name, nargs in ARGS.items():
        assert hasattr(raw, name), "libadacodec.so does not export %s" % name
        assert name in adac.SIGNATURES and len(adac.SIGNATURES[name][1]) == nargs, name
    for method in ("scan_sum", "scan_count_between", "scan_select_between", "scan_min_max"):
        assert callable(getattr(adac.BitpackingLayout, method)), method
    assert isinstance(adac.BitpackingLayout.value_span, property)
    assert lib.adac_abi_version() == 1
    # a NULL layout is an argument error, not a crash (no device is touched)
    assert raw.adac_bp_scan_sum(None, None, None, None) == 1
    assert raw.adac_bp_scan_min_max(None, None, None, None) == 1
    raw.adac_bp_layout_value_span.restype = C.c_uint64
    assert raw.adac_bp_layout_value_span(None) == 0


def test_scan_kernels_have_no_spills_and_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = {k: v for k, v in kr.parse().items() if k.startswith("k_bp_scan")}
    assert table, "no k_bp_scan kernel in the build's resource remarks"
    assert any(k.startswith("k_bp_scan<") for k in table)
    for name, r in table.items():
        assert r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
    # and tests/test_kernel_budget.py holds their registers, LDS and occupancy against profiles/kernel_budget.json
    # (all but the one-thread-per-segment k_bp_scan_minmax_finish)
    assert all(k.startswith(kr.BUDGETED) for k in table if k != "k_bp_scan_minmax_finish")
