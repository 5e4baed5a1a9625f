"""adac_bp_unpack_selected as an interface (no GPU): the header declares it, the library exports it, the Python binding
carries it, a NULL layout is an argument error, and the compiler's resource remarks show the new kernels free of
spills and scratch."""
import ctypes as C
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, NARGS = "adac_bp_unpack_selected", 6
KERNELS = ("k_bp_gather<", "k_bp_group_popc")


@pytest.fixture(scope="module")
def lib(adac):
    adac.build()
    return adac.lib()


def test_header_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "#define ADAC_ABI_VERSION 1" in hdr
    m = re.search(r"\badac_status\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert m, NAME
    assert len(m.group(1).split(",")) == NARGS, m.group(1)


def test_library_exports_and_binding_holds_it(adac, lib):
    raw = C.CDLL(adac.LIB_PATH)
    assert hasattr(raw, NAME), "libadacodec.so does not export %s" % NAME
    assert NAME in adac.SIGNATURES and len(adac.SIGNATURES[NAME][1]) == NARGS
    assert callable(getattr(adac.BitpackingLayout, "unpack_selected"))
    assert lib.adac_abi_version() == 1
    # a NULL layout is an argument error, not a crash (no device is touched)
    assert raw.adac_bp_unpack_selected(None, None, None, None, None, None) == 1
    total = C.c_uint64(77)
    assert lib.adac_bp_unpack_selected(None, None, None, None, None, C.byref(total)) == 1
    assert total.value == 77


def test_gather_kernels_have_no_spills_and_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = {k: v for k, v in kr.parse().items() if k.startswith(KERNELS)}
    # the gather per type size, without and with the ids; one count kernel
    want = ["k_bp_gather<%s,%s>" % (u, ids) for u in ("u8", "u16", "u32", "u64") for ids in ("false", "true")]
    assert sorted(table) == sorted(want + ["k_bp_group_popc"]), sorted(table)
    for name, r in table.items():
        assert r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
    # and tests/test_kernel_budget.py holds their registers, LDS and occupancy against profiles/kernel_budget.json
    assert all(k.startswith(kr.BUDGETED) for k in table)
