"""The owner of the library's device buffers (csrc/adac_owned.h) and the scan-group deal (csrc/adac_scan_deal.h) as a
stand-alone host program under AddressSanitizer and UBSan: no GPU, nothing loaded into Python.
tests/owned_groups_check.cpp defines the owner's memory calls over a counting allocator that refuses the k-th
allocation and holds the checks: for every k of every group a layout allocates, no member is set after the failure,
nothing leaks or is freed twice (the sanitizer's exit status decides), a second attempt succeeds; moves leave the
source empty and free the destination's old buffer once; a request for no elements yields one.  The deal: the groups
of a segment are in order and partition it, none exceeds 65,536 rows, seg_groups is their number, and every bitmap word
that groups cover in part has one cell that all its arrivals share, each expecting as many arrivals as there are."""
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "duckdb-adaptive-compression_amd"
forms = importlib.import_module(PKG + ".forms")  # host-only module: no library is loaded


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("owned_groups") / "owned_groups_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, PKG, "csrc"), os.path.join(ROOT, "tests", "owned_groups_check.cpp"),
                           "-o", exe])
    return exe


def run(prog, *args):
    p = subprocess.run([prog, *map(str, args)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_owner_groups_and_deal_hold_every_invariant(prog):
    assert run(prog).strip() == "ok"


@pytest.mark.parametrize("type_size", [1, 2, 4, 8])
def test_default_tiles_per_group_match_the_form_mirror(prog, type_size):
    assert int(run(prog, "per", type_size)) == forms.TILES_PER_SCAN_GROUP[type_size]
