"""adac_bp_scan_select_compare / adac_bp_scan_count_compare as an interface (no GPU): the header declares them, the
library exports them, the Python binding carries them, a NULL layout is an argument error, and the compiler's resource
remarks show the new kernel free of spills and scratch."""
import ctypes as C
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"adac_bp_scan_select_compare": 8, "adac_bp_scan_count_compare": 7}
KERNEL = "k_bp_scan_pair_cmp<"


@pytest.fixture(scope="module")
def lib(adac):
    adac.build()
    return adac.lib()


def test_header_declares_both_entry_points_and_the_three_bits():
    hdr = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "#define ADAC_ABI_VERSION 1" in hdr
    for name, nargs in ARGS.items():
        m = re.search(r"\badac_status\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    assert re.search(r"ADAC_CMP_LT\s*=\s*1\s*,\s*ADAC_CMP_EQ\s*=\s*2\s*,\s*ADAC_CMP_GT\s*=\s*4\b", hdr)


def test_library_exports_and_binding_holds_them(adac, lib):
    raw = C.CDLL(adac.LIB_PATH)
    for name, nargs in ARGS.items():
        assert hasattr(raw, name), "libadacodec.so does not export %s" % name
        assert name in adac.SIGNATURES and len(adac.SIGNATURES[name][1]) == nargs, name
    for method in ("scan_select_compare", "scan_count_compare"):
        assert callable(getattr(adac.BitpackingLayout, method)), method
    assert (adac.CMP_LT, adac.CMP_EQ, adac.CMP_GT, adac.CMP_LE, adac.CMP_NE, adac.CMP_GE) == (1, 2, 4, 3, 5, 6)
    assert lib.adac_abi_version() == 1
    # a NULL layout is an argument error, not a crash (no device is touched)
    assert raw.adac_bp_scan_select_compare(None, None, None, None, None, 1, None, None) == 1
    assert raw.adac_bp_scan_count_compare(None, None, None, None, None, 1, None) == 1


def test_compare_kernel_has_no_spills_and_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = {k: v for k, v in kr.parse().items() if k.startswith(KERNEL)}
    # masked and unmasked form
    assert sorted(table) == [KERNEL + "false>", KERNEL + "true>"], sorted(table)
    for name, r in table.items():
        assert r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
    # and tests/test_kernel_budget.py holds their registers, LDS and occupancy against profiles/kernel_budget.json
    assert all(k.startswith(kr.BUDGETED) for k in table)
