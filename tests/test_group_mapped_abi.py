"""adac_scan_group_sum_mapped / adac_scan_group_count_mapped / adac_scan_build_map as an interface (no GPU): the header
declares them with their argument lists, the library exports them, the Python binding carries them, a NULL layout is an
argument error, the ABI version is still 1, the knob exists, and the compiler's resource remarks show exactly the
expected kernels, free of VGPR spills and scratch and held by the budget."""
import ctypes as C
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "adac_scan_group_sum_mapped": [
        "adac_layout *keys", "const uint64_t *d_key_words", "adac_layout *values", "const uint64_t *d_value_words",
        "const uint64_t *d_validity", "const uint8_t *d_map", "uint64_t key_base", "uint64_t key_span", "uint32_t ngroups",
        "uint64_t *d_sums", "uint64_t *d_counts", "uint64_t *d_seg_rows"],
    "adac_scan_group_count_mapped": [
        "adac_layout *keys", "const uint64_t *d_key_words", "const uint64_t *d_validity", "const uint8_t *d_map",
        "uint64_t key_base", "uint64_t key_span", "uint32_t ngroups", "uint64_t *d_counts", "uint64_t *d_seg_rows"],
    "adac_scan_build_map": [
        "adac_layout *keys", "const uint64_t *d_key_words", "adac_layout *codes", "const uint64_t *d_code_words",
        "const uint64_t *d_validity", "uint64_t key_base", "uint64_t key_span", "uint32_t fill", "uint8_t *d_map",
        "uint64_t *d_seg_rows"],
}
# <mask given, value column read> and <mask given>
KERNELS = ["k_group_mapped<%s,%s>" % (v, s) for v in ("false", "true") for s in ("false", "true")] + \
          ["k_build_map<%s>" % v for v in ("false", "true")]


@pytest.fixture(scope="module")
def lib(adac):
    adac.build()
    return adac.lib()


def test_header_declares_the_three_entry_points():
    hdr = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    assert '"group_mapped_copies"' in hdr  # the knob list
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "#define ADAC_ABI_VERSION 1" in hdr
    for name, want in ARGS.items():
        m = re.search(r"\badac_status\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert args == want, (name, args)


def test_library_exports_and_binding_holds_them(adac, lib):
    raw = C.CDLL(adac.LIB_PATH)
    for name, want in ARGS.items():
        assert hasattr(raw, name), "libadacodec.so does not export %s" % name
        assert name in adac.SIGNATURES and len(adac.SIGNATURES[name][1]) == len(want), name
    for method in ("scan_group_sum_mapped", "scan_group_count_mapped", "scan_build_map"):
        assert callable(getattr(adac.Layout, method)), method
    assert lib.adac_abi_version() == 1
    # a NULL layout is an argument error, not a crash (no device is touched)
    assert lib.adac_scan_group_sum_mapped(None, None, None, None, None, None, 0, 1, 1, None, None, None) == 1
    assert lib.adac_scan_group_count_mapped(None, None, None, None, 0, 1, 1, None, None) == 1
    assert lib.adac_scan_build_map(None, None, None, None, None, 0, 1, 255, None, None) == 1
    # the knob: known, refuses a negative number of copies, and back at its default
    assert lib.adac_set_tuning(b"group_mapped_copies", 1) == 0
    assert lib.adac_set_tuning(b"group_mapped_copies", -1) != 0
    assert lib.adac_set_tuning(b"group_mapped_copies", 0) == 0


def test_mapped_kernels_have_no_vgpr_spills_and_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = {k: v for k, v in kr.parse().items() if k.startswith(("k_group_mapped<", "k_build_map<"))}
    assert sorted(table) == sorted(KERNELS), sorted(table)
    for name, r in table.items():
        assert r["vgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds"] <= 18 * 1024, (name, r)   # eight workgroups per CU
    # and tests/test_kernel_budget.py holds their registers, LDS and occupancy against profiles/kernel_budget.json
    assert all(k.startswith(kr.BUDGETED) for k in table)
    budget = json.load(open(kr.BUDGET))["kernels"]
    assert all(k in budget for k in table)
