"""The infill without a GPU: its numpy restatement (tests/infill_reference.py) against the recorded first-hit histograms,
csrc/infill_math.hpp compiled for the CPU against the restatement's candidate order, the public header as C99, and what
the built library exports and holds."""
import os
import re
import subprocess

import numpy as np
import pytest

import infill_reference as ir
import zoom_reference as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
CHECK = os.path.join(ROOT, "tests", "cpu_device", "infill_math_check.cpp")


def test_restatement_reproduces_the_recorded_first_hit_histograms():
    n = len(zr.TIMES)
    res = ir.nine_frames()
    assert len(ir.HISTOGRAMS) == len(ir.LEFT_FOR_FILL) == len(ir.ORDER_SENSITIVE) == n
    for f, (place, pos, both) in enumerate(res):
        cand = ir.candidates(f, n, ir.RADIUS)
        hist, left = ir.histogram(place, len(cand))
        print(f, cand, hist, left, int(both.sum()))
        assert tuple(hist) == ir.HISTOGRAMS[f] and left == ir.LEFT_FOR_FILL[f]
        assert sum(hist) + left == place.size
        assert min(hist) >= 5, (f, hist)                                  # every candidate of every frame is a first hit
        assert int(both.sum()) == ir.ORDER_SENSITIVE[f]
        assert np.isnan(pos[place < 0]).all() and np.isfinite(pos[place >= 0]).all()
    assert ir.HISTOGRAMS[4] == (246304, 250, 6304, 140, 2446, 198, 61) and ir.LEFT_FOR_FILL[4] == 1177
    assert [ir.ORDER_SENSITIVE[f] for f in (2, 3, 6, 7)] == [5207, 126, 10, 148]


def test_candidate_order_of_the_restatement():
    assert ir.candidates(4, 9, 3) == [4, 3, 5, 2, 6, 1, 7]
    assert ir.candidates(0, 9, 3) == [0, 1, 2, 3]
    assert ir.candidates(8, 9, 3) == [8, 7, 6, 5]
    assert ir.candidates(1, 9, 3) == [1, 0, 2, 3, 4]
    assert ir.candidates(2, 3, 8) == [2, 1, 0]
    assert ir.candidates(5, 9, 0) == [5] and ir.candidates(0, 1, 8) == [0]
    from rssync_amd import infill
    for n in (1, 2, 9):
        for f in range(n):
            for r in (0, 1, 3, 8):
                assert infill.candidates(f, n, r) == ir.candidates(f, n, r)


def _run_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, CHECK], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout


def test_header_candidate_order_is_the_restatements(tmp_path):
    plain = _run_check(tmp_path, "plain", [])
    # host code in a stand-alone program: the sanitizers' runtimes are linked in, nothing is preloaded
    checked = _run_check(tmp_path, "sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert plain == checked, "the sanitized build printed something else"
    assert "mismatch" not in plain
    want = []
    for n in range(1, 21):
        for f in range(n):
            for radius in range(9):
                want.append("c %d %d %d :%s" % (n, f, radius, "".join(" %d" % g for g in ir.candidates(f, n, radius))))
    assert plain.splitlines() == want
    assert len(want) == 9 * sum(range(1, 21))


def test_public_header_is_c99(tmp_path):
    src = tmp_path / "infill.c"
    src.write_text('#include "rssync_infill.h"\n'
                   'int main(void) { return RSSYNC_INFILL_MAX_RADIUS == 8 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o",
                    str(tmp_path / "infill.o"), str(src)], check=True)


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


INFILL_KERNELS = ["infill_rows_kernel"] + ["infill_kernelILi%dELi%dE" % (c, f) for c in (0, 1) for f in (0, 1)]
OTHER_FAMILIES = ("stabilize", "rectify", "zoom", "bicubic", "limit_", "color_", "color16_", "percam_")


def test_library_exports_the_infill_and_holds_its_kernels(built, tmp_path):
    import rssync_amd
    from rssync_amd import infill
    lib = rssync_amd.library_path()
    text = open(os.path.join(ROOT, "include", "rssync_infill.h")).read()
    declared = set(re.findall(r"\b(rssync_infill_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == {"rssync_infill_stabilize"}
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {e for e in exported if e.startswith("rssync_infill_")} == declared
    assert {e for e in exported if e.startswith("rship_infill_")} == {"rship_infill_frames"}
    assert declared <= set(infill.SIGNATURES) and "rship_infill_frames" in infill.SIGNATURES
    infill.library()                    # binds every signature: a missing symbol raises
    for name in ("stabilize_frames_infilled", "stabilize_frames_infilled_budget"):
        assert callable(getattr(rssync_amd.SyncProblem, name)) and callable(getattr(infill, name))
    # the code object: every kernel of the infill is there, once, and needs neither scratch nor spills
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "infill" in name.lower():
            found[name] = {k: int(re.search(r"\.%s:\s+(\S+)" % k, block).group(1))
                           for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    for want in INFILL_KERNELS:
        hit = [n for n in found if want in n]
        assert len(hit) == 1, (want, sorted(found))
        print(want, found[hit[0]])
    assert len(found) == len(INFILL_KERNELS), sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        # the kernel's name and its argument struct's, which is part of it: of no family that other tests count
        assert not any(fam in name.lower() for fam in OTHER_FAMILIES), name
