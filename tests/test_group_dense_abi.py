"""adac_scan_group_sum_dense / adac_scan_group_count_dense as an interface (no GPU): the header declares them, the
library exports them, the Python binding carries them, a NULL layout is an argument error, the ABI version is still 1,
the knob exists, and the compiler's resource remarks show the four kernels free of VGPR spills and scratch."""
import ctypes as C
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"adac_scan_group_sum_dense": 10, "adac_scan_group_count_dense": 7}
KERNELS = ["k_group_dense<%s,%s>" % (v, s) for v in ("false", "true") for s in ("false", "true")]


@pytest.fixture(scope="module")
def lib(adac):
    adac.build()
    return adac.lib()


def test_header_declares_the_two_entry_points():
    hdr = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    assert '"group_dense_combine"' in hdr  # the knob list
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "#define ADAC_ABI_VERSION 1" in hdr
    for name, nargs in ARGS.items():
        m = re.search(r"\badac_status\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs, (name, args)
        assert args[0] == "adac_layout *keys" and args[1] == "const uint64_t *d_key_words"
        assert "uint64_t key_base" in args and "uint64_t key_span" in args and "const uint64_t *d_validity" in args
        assert ("adac_layout *values" in args) == (name == "adac_scan_group_sum_dense")
        assert ("uint64_t *d_sums" in args) == (name == "adac_scan_group_sum_dense")
        assert args[-2] == "uint64_t *d_counts" and args[-1] == "uint64_t *d_seg_rows"


def test_library_exports_and_binding_holds_them(adac, lib):
    raw = C.CDLL(adac.LIB_PATH)
    for name, nargs in ARGS.items():
        assert hasattr(raw, name), "libadacodec.so does not export %s" % name
        assert name in adac.SIGNATURES and len(adac.SIGNATURES[name][1]) == nargs, name
    for method in ("scan_group_sum_dense", "scan_group_count_dense"):
        assert callable(getattr(adac.Layout, method)), method
    assert lib.adac_abi_version() == 1
    # a NULL layout is an argument error, not a crash (no device is touched)
    assert lib.adac_scan_group_sum_dense(None, None, None, None, None, 0, 1, None, None, None) == 1
    assert lib.adac_scan_group_count_dense(None, None, None, 0, 1, None, None) == 1
    # the knob: known, and back at its default
    assert lib.adac_set_tuning(b"group_dense_combine", 0) == 0
    assert lib.adac_set_tuning(b"group_dense_combine", 1) == 0


def test_dense_kernels_have_no_vgpr_spills_and_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = {k: v for k, v in kr.parse().items() if k.startswith("k_group_dense<")}
    # <mask given, value column read>
    assert sorted(table) == sorted(KERNELS), sorted(table)
    for name, r in table.items():
        assert r["vgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds"] <= 18 * 1024, (name, r)   # eight workgroups per CU
    # and tests/test_kernel_budget.py holds their registers, LDS and occupancy against profiles/kernel_budget.json
    assert all(k.startswith(kr.BUDGETED) for k in table)
    budget = json.load(open(kr.BUDGET))["kernels"]
    assert all(k in budget for k in table)
