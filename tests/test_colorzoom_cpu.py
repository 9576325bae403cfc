"""The dynamic zoom for colour video without a GPU (include/rssync_colorzoom.h): the public header as C99, what the built
library declares, exports and binds, and the code object's kernels of csrc/kernels/colorzoom.hpp: all 28 instantiations,
each once, without a private segment and without spills."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"

FUNCTIONS = {"rssync_colorzoom_stabilize", "rssync_colorzoom_fit"}

# <CAMERA, NV12, FILTER>, <CAMERA, FILTER>, <CAMERA, SEMI, SHIFT, FILTER> (P010, P016, I010), <CAMERA, FILTER>
KERNELS = ["percam_yuv8_kernelILi%dELb%dELi%dE" % (c, nv, f) for c in (0, 1) for nv in (0, 1) for f in (0, 1)]
KERNELS += ["percam_rgba8_kernelILi%dELi%dE" % (c, f) for c in (0, 1) for f in (0, 1)]
KERNELS += ["percam_yuv16_kernelILi%dELb%dELi%dELi%dE" % (c, semi, shift, f) for c in (0, 1) for semi, shift in ((1, 6), (1, 0), (0, 0))
            for f in (0, 1)]
KERNELS += ["percam_gray16_kernelILi%dELi%dE" % (c, f) for c in (0, 1) for f in (0, 1)]


def test_public_header_is_c99(tmp_path):
    src = tmp_path / "colorzoom.c"
    src.write_text('#include "rssync_colorzoom.h"\n'
                   "int use(rssync_problem* p, const rssync_color_image* a, const rssync_color_image* b, const double* t, const rssync_lens* l,\n"
                   "        double* z, uint32_t* s) {\n"
                   "    rssync_color_params q = {0};\n"
                   "    return rssync_colorzoom_fit(p, RSSYNC_COLOR16_P010, 4, 4, l, 4, 4, t, 1, 0.0, 0, &q, 1.0, 1.5, 0, z, s) == RSSYNC_ZOOM_CLEAR\n"
                   "        ? rssync_colorzoom_stabilize(p, RSSYNC_COLOR_NV12, a, 1, 4, 4, t, l, 0.0, 0, &q, b, 4, 4, 0, z) : -1;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o",
                    str(tmp_path / "colorzoom.o"), str(src)], check=True)


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


def test_declared_exported_and_bound_functions_are_the_two(built):
    import rssync_amd
    from rssync_amd import colorzoom
    text = open(os.path.join(ROOT, "include", "rssync_colorzoom.h")).read()
    declared = set(re.findall(r"\b(rssync_colorzoom_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == FUNCTIONS
    nm = subprocess.check_output(["nm", "-D", "--defined-only", rssync_amd.library_path()], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {e for e in exported if e.startswith("rssync_colorzoom")} == FUNCTIONS
    assert "rship_colorzoom_frames" in exported
    assert {name for name in colorzoom.SIGNATURES if name.startswith("rssync_colorzoom")} == FUNCTIONS
    colorzoom.library()                 # binds every signature: a missing symbol raises
    for name in ("stabilize_color_zoomed", "stabilize_color_zoomed_budget", "fit_zoom_color", "dynamic_zoom_color"):
        assert callable(getattr(rssync_amd.SyncProblem, name)) and callable(getattr(colorzoom, name))


def test_library_holds_every_kernel_once_without_scratch_or_spills(built, tmp_path):
    import rssync_amd
    lib = rssync_amd.library_path()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "percam_" in name:
            found[name] = {k: int(re.search(r"\.%s:\s+(\S+)" % k, block).group(1))
                           for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    assert len(KERNELS) == 28
    for want in KERNELS:
        hit = [n for n in found if want in n]
        assert len(hit) == 1, (want, sorted(found))
        print(want, found[hit[0]])
    assert len(found) == len(KERNELS), sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
