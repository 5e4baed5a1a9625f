"""adac_scan_select_member / adac_scan_count_member / adac_scan_build_member as an interface (no GPU): the header
declares them, the library exports them, the Python binding carries them, a NULL layout is an argument error, the ABI
version is still 1, and the compiler's resource remarks show the new kernels free of VGPR spills and scratch."""
import ctypes as C
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"adac_scan_select_member": 8, "adac_scan_count_member": 7, "adac_scan_build_member": 7}
KERNELS = ["k_scan_member<%s,%s>" % (v, s) for v in ("false", "true") for s in ("false", "true")] + \
          ["k_scan_member_build<%s>" % v for v in ("false", "true")]


@pytest.fixture(scope="module")
def lib(adac):
    adac.build()
    return adac.lib()


def test_header_declares_the_three_entry_points():
    hdr = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "#define ADAC_ABI_VERSION 1" in hdr
    for name, nargs in ARGS.items():
        m = re.search(r"\badac_status\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs, (name, args)
        assert args[0] == "adac_layout *l" and "uint64_t set_base" in args and "uint64_t set_bits" in args
        assert ("const uint64_t *d_set" in args) == (name != "adac_scan_build_member")
        assert ("uint64_t *d_set" in args) == (name == "adac_scan_build_member")
        assert ("uint64_t *d_bitmap" in args) == (name == "adac_scan_select_member")
        assert args[-1] == "uint64_t *d_counts"


def test_library_exports_and_binding_holds_them(adac, lib):
    raw = C.CDLL(adac.LIB_PATH)
    for name, nargs in ARGS.items():
        assert hasattr(raw, name), "libadacodec.so does not export %s" % name
        assert name in adac.SIGNATURES and len(adac.SIGNATURES[name][1]) == nargs, name
    for method in ("scan_select_member", "scan_count_member", "scan_build_member"):
        assert callable(getattr(adac.Layout, method)), method
    assert lib.adac_abi_version() == 1
    # a NULL layout is an argument error, not a crash (no device is touched)
    assert lib.adac_scan_select_member(None, None, None, None, 0, 1, None, None) == 1
    assert lib.adac_scan_count_member(None, None, None, None, 0, 1, None) == 1
    assert lib.adac_scan_build_member(None, None, None, 0, 1, None, None) == 1


def test_member_kernels_have_no_vgpr_spills_and_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = {k: v for k, v in kr.parse().items() if k.startswith("k_scan_member")}
    # probe: <mask given, bitmap written>; build: <mask given>
    assert sorted(table) == sorted(KERNELS), sorted(table)
    for name, r in table.items():
        assert r["vgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds"] <= 18 * 1024, (name, r)   # eight workgroups per CU
    # and tests/test_kernel_budget.py holds their registers, LDS and occupancy against profiles/kernel_budget.json
    assert all(k.startswith(kr.BUDGETED) for k in table)
    budget = json.load(open(kr.BUDGET))["kernels"]
    assert all(k in budget for k in table)
