"""The pair scans on BITPACKING blocks as an interface (no GPU): the header declares them, the library exports them,
the Python binding carries them, a NULL layout is an argument error, and the compiler's resource remarks show the new
kernels free of spills and scratch."""
import ctypes as C
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"adac_bp_scan_sum_product": 6, "adac_bp_scan_group_sum": 8}
KERNELS = ("k_bp_scan_pair_sum<", "k_bp_scan_pair_gsum<")


@pytest.fixture(scope="module")
def lib(adac):
    adac.build()
    return adac.lib()


def test_header_declares_both_entry_points():
    hdr = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "#define ADAC_ABI_VERSION 1" in hdr
    for name, nargs in ARGS.items():
        m = re.search(r"\badac_status\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))


def test_library_exports_and_binding_holds_them(adac, lib):
    raw = C.CDLL(adac.LIB_PATH)
    for name, nargs in ARGS.items():
        assert hasattr(raw, name), "libadacodec.so does not export %s" % name
        assert name in adac.SIGNATURES and len(adac.SIGNATURES[name][1]) == nargs, name
    for method in ("scan_sum_product", "scan_group_sum"):
        assert callable(getattr(adac.BitpackingLayout, method)), method
    assert lib.adac_abi_version() == 1
    # a NULL layout is an argument error, not a crash (no device is touched)
    assert raw.adac_bp_scan_sum_product(None, None, None, None, None, None) == 1
    assert raw.adac_bp_scan_group_sum(None, None, None, None, None, 6, None, None) == 1


def test_pair_scan_kernels_have_no_spills_and_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = {k: v for k, v in kr.parse().items() if k.startswith(KERNELS)}
    # masked and unmasked form of each
    assert sorted(table) == sorted(k + v + ">" for k in KERNELS for v in ("false", "true")), sorted(table)
    for name, r in table.items():
        assert r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
    # and tests/test_kernel_budget.py holds their registers, LDS and occupancy against profiles/kernel_budget.json
    assert all(k.startswith(kr.BUDGETED) for k in table)
