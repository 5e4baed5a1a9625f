"""adac_scan_select_compare / adac_scan_count_compare as an interface (no GPU): the header declares them, the library
exports them, the Python binding carries them, a NULL layout is an argument error, and the compiler's resource remarks
show the four instantiations of the new kernel free of VGPR spills and scratch."""
import ctypes as C
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"adac_scan_select_compare": 8, "adac_scan_count_compare": 7}
KERNEL = "k_scan_compare<"


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
        assert "adac_layout *a" in m.group(1) and "adac_layout *b" in m.group(1) and "uint32_t cmp" in m.group(1)
    assert re.search(r"ADAC_CMP_LT\s*=\s*1\s*,\s*ADAC_CMP_EQ\s*=\s*2\s*,\s*ADAC_CMP_GT\s*=\s*4\b", hdr)


def test_library_exports_and_binding_holds_them(adac, lib):
    raw = C.CDLL(adac.LIB_PATH)
    for name, nargs in ARGS.items():
        assert hasattr(raw, name), "libadacodec.so does not export %s" % name
        assert name in adac.SIGNATURES and len(adac.SIGNATURES[name][1]) == nargs, name
    for method in ("scan_select_compare", "scan_count_compare"):
        assert callable(getattr(adac.Layout, method)), method
    assert (adac.CMP_LT, adac.CMP_EQ, adac.CMP_GT, adac.CMP_LE, adac.CMP_NE, adac.CMP_GE) == (1, 2, 4, 3, 5, 6)
    assert lib.adac_abi_version() == 1
    # a NULL layout is an argument error, not a crash (no device is touched)
    assert raw.adac_scan_select_compare(None, None, None, None, None, 1, None, None) == 1
    assert raw.adac_scan_count_compare(None, None, None, None, None, 1, None) == 1


def test_compare_kernel_has_no_vgpr_spills_and_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = {k: v for k, v in kr.parse().items() if k.startswith(KERNEL)}
    # <mask given, bitmap written>
    assert sorted(table) == [KERNEL + "%s,%s>" % (v, s) for v in ("false", "true") for s in ("false", "true")], sorted(table)
    for name, r in table.items():
        assert r["vgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
    # and tests/test_kernel_budget.py holds their registers, LDS and occupancy against profiles/kernel_budget.json
    assert all(k.startswith(kr.BUDGETED) for k in table)
    import json
    budget = json.load(open(kr.BUDGET))["kernels"]
    assert all(k in budget for k in table)
