"""adac_scan_group_sum_product_mapped as an interface (no GPU): the header declares it with its argument list, the library
exports it, the Python binding carries it, a NULL layout is an argument error, the ABI version is still 1, and the
compiler's resource remarks show exactly the expected instantiations of the kernel, free of VGPR spills and scratch, at
the residency its file states, and held by the budget."""
import ctypes as C
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "adac_scan_group_sum_product_mapped"
ARGS = ["adac_layout *keys", "const uint64_t *d_key_words", "adac_layout *a", "const uint64_t *d_a_words",
        "adac_layout *b", "const uint64_t *d_b_words", "const uint64_t *d_validity", "const uint8_t *d_map",
        "uint64_t key_base", "uint64_t key_span", "uint32_t ngroups", "uint64_t *d_sums_ab", "uint64_t *d_sums_a",
        "uint64_t *d_counts", "uint64_t *d_seg_rows"]
# <mask given, d_sums_a wanted>
KERNELS = ["k_group_mapped_product<%s,%s>" % (v, a) for v in ("false", "true") for a in ("false", "true")]


@pytest.fixture(scope="module")
def lib(adac):
    adac.build()
    return adac.lib()


def test_header_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    assert "100 * d_sums_a[g] - d_sums_ab[g]" in hdr   # the Q5 recipe
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "#define ADAC_ABI_VERSION 1" in hdr
    m = re.search(r"\badac_status\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert m, NAME
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ARGS, args


def test_library_exports_and_binding_holds_it(adac, lib):
    raw = C.CDLL(adac.LIB_PATH)
    assert hasattr(raw, NAME), "libadacodec.so does not export %s" % NAME
    assert NAME in adac.SIGNATURES and len(adac.SIGNATURES[NAME][1]) == len(ARGS)
    assert callable(getattr(adac.Layout, "scan_group_sum_product_mapped"))
    assert lib.adac_abi_version() == 1
    # a NULL layout is an argument error, not a crash (no device is touched)
    assert getattr(lib, NAME)(None, None, None, None, None, None, None, None, 0, 1, 1, None, None, None, None) == 1


def test_the_kernel_has_no_vgpr_spills_and_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = {k: v for k, v in kr.parse().items() if k.startswith("k_group_mapped_product<")}
    assert sorted(table) == sorted(KERNELS), sorted(table)
    src = open(os.path.join(ROOT, "duckdb-adaptive-compression_amd", "csrc", "adac_group_mapped_product.inl")).read()
    resident = int(re.search(r"constexpr uint32_t kMappedProductResident = (\d+);", src).group(1))
    for name, r in table.items():
        assert r["vgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds"] * resident <= 160 * 1024, (name, r)   # the workgroups per CU the file states, by LDS ...
        assert r["occupancy"] >= resident, (name, r)          # ... and by registers (waves per SIMD)
    # and tests/test_kernel_budget.py holds their registers, LDS and occupancy against profiles/kernel_budget.json
    assert all(k.startswith(kr.BUDGETED) for k in table)
    budget = json.load(open(kr.BUDGET))["kernels"]
    assert all(k in budget for k in table)
