"""adac_scan_group_sum_q1 exists in every layer a caller meets — header, library, ctypes table, Layout, tuning knob — and
its kernels, masked and unmasked, are budgeted without spills or scratch.  No GPU needed.

The numpy reference of the GPU tests (tests/test_gpu_group_sum_q1.py) is checked against Python integers here."""
import ctypes
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TERMS = ("ADAC_Q1_COUNT", "ADAC_Q1_SUM_Q", "ADAC_Q1_SUM_A", "ADAC_Q1_SUM_B", "ADAC_Q1_SUM_AB", "ADAC_Q1_SUM_AC",
         "ADAC_Q1_SUM_ABC")


def test_header_declares_the_entry_point_the_terms_and_the_knob():
    text = open(os.path.join(ROOT, "include", "adacodec.h")).read()
    m = re.search(r"adac_status\s+adac_scan_group_sum_q1\s*\(([^)]*)\)\s*;", text)
    assert m, "include/adacodec.h does not declare adac_scan_group_sum_q1"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 13
    for i, name in ((0, "*a"), (2, "*b"), (4, "*c"), (6, "*q"), (8, "*keys")):
        assert "adac_layout" in params[i] and params[i].endswith(name), params[i]
    for i, name in ((1, "d_a_words"), (3, "d_b_words"), (5, "d_c_words"), (7, "d_q_words"), (9, "d_key_words"),
                    (10, "d_validity")):
        assert "const uint64_t" in params[i] and params[i].endswith(name), params[i]
    assert params[11] == "uint32_t ngroups" and params[12] == "uint64_t *d_out"
    assert re.search(r"#define\s+ADAC_Q1_TERMS\s+7\b", text)
    for value, name in enumerate(TERMS):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text), name
    assert '"group_q1_rw"' in text  # the knob list
    handover = text[text.index("Diagnostic, not part of the drop-in boundary: *left"):]
    assert "adac_scan_group_sum_q1" in handover[:handover.index("adac_debug_group_handover(")]


def test_library_exports_the_entry_point(adac):
    lib = ctypes.CDLL(adac.build())
    assert hasattr(lib, "adac_scan_group_sum_q1")
    assert adac.lib().adac_abi_version() == 1  # an added entry point is compatible


def test_signature_has_thirteen_arguments(adac):
    res, args = adac.SIGNATURES["adac_scan_group_sum_q1"]
    assert res is ctypes.c_int and len(args) == 13
    assert args[11] is ctypes.c_uint32
    assert all(ctypes.sizeof(a) == ctypes.sizeof(ctypes.c_void_p) for i, a in enumerate(args) if i != 11)


def test_layout_has_the_method_and_the_term_indices(adac):
    assert callable(getattr(adac.Layout, "scan_group_sum_q1"))
    assert adac.Q1_TERMS == 7
    assert [adac.Q1_COUNT, adac.Q1_SUM_Q, adac.Q1_SUM_A, adac.Q1_SUM_B, adac.Q1_SUM_AB, adac.Q1_SUM_AC,
            adac.Q1_SUM_ABC] == list(range(7))


def test_the_knob_is_known(adac):
    adac.build()
    try:
        assert adac.lib().adac_set_tuning(b"group_q1_rw", 0) == 0
    finally:
        assert adac.lib().adac_set_tuning(b"group_q1_rw", 1) == 0


def test_q1_kernels_are_budgeted_masked_and_unmasked(adac):
    import kernel_resources as kr
    adac.build()
    assert "k_group_q1" in kr.BUDGETED
    mine = {k: v for k, v in kr.budgeted(kr.parse()).items() if k.startswith("k_group_q1")}
    for name in ("k_group_q1_rw<false>", "k_group_q1_rw<true>", "k_group_q1<false>", "k_group_q1<true>"):
        assert name in mine, sorted(mine)
    for name, r in mine.items():
        assert r["vgpr_spills"] == 0 and r["scratch"] == 0, (name, r)
    committed = json.load(open(os.path.join(ROOT, "profiles", "kernel_budget.json")))["kernels"]
    assert set(mine) <= set(committed), sorted(set(mine) - set(committed))
    for name in mine:
        assert committed[name]["vgpr_spills"] == 0 and committed[name]["scratch"] == 0, name


def test_the_numpy_reference_is_python_integer_arithmetic_mod_2_64():
    """reference_q1 of tests/test_gpu_group_sum_q1.py — the seven terms per bin from the widened uint64 columns —
    equals Python integers taken mod 2^64, with negative values and products that wrap"""
    from test_gpu_group_sum_q1 import reference_q1
    rng = np.random.default_rng(17)
    n = 1000
    types = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
    wrapped = negative = 0
    for i in range(len(types)):
        cols = []
        for shift in (0, 3, 5, 6):
            t = np.dtype(types[(i + shift) % len(types)])
            info = np.iinfo(t)
            v = rng.integers(info.min, info.max, size=n, dtype=t, endpoint=True)
            v[:4] = [info.min, info.max, info.min, info.max]
            cols.append(v)
        a, b, c, q = cols
        keys = rng.integers(0, 12, size=n).astype(np.uint16)
        keep = rng.random(n) < 0.6
        for ngroups, mask in ((7, None), (7, keep), (200, keep)):
            got = reference_q1(a, b, c, q, keys, ngroups, mask)
            want = [[0] * (ngroups + 1) for _ in range(7)]
            for r in range(n):
                if mask is not None and not mask[r]:
                    continue
                x, y, z, v = int(a[r]), int(b[r]), int(c[r]), int(q[r])
                g = min(int(keys[r]), ngroups)
                for t, add in enumerate((1, v, x, y, x * y, x * z, x * y * z)):
                    want[t][g] = (want[t][g] + add) % 2 ** 64
            assert got == want, (i, ngroups, mask is not None)
        wrapped += sum(1 for r in range(n) if abs(int(a[r]) * int(b[r]) * int(c[r])) >= 2 ** 64)
        negative += sum(1 for r in range(n) if int(a[r]) * int(b[r]) < 0)
    assert wrapped > 1000 and negative > 1000
