"""The dynamic zoom for 4:2:2 and 4:4:4 video without a GPU (include/rssync_zoomyuv.h): the public header as C99, what the
built library declares, exports and binds, the code object's kernels of csrc/kernels/zoomyuv.hpp -- all 28 instantiations,
each once, without a private segment and without spills --, and the numpy statement of the fit with the domination pattern
that tests/test_gpu_zoomyuv.py's guard relies on."""
import os
import re
import subprocess

import numpy as np
import pytest

import rectify_reference as rr
import stabilize_reference as sr
import yuv_reference as yr
import zoom_reference as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"

FUNCTIONS = {"rssync_zoomyuv_stabilize", "rssync_zoomyuv_fit"}

# <CAMERA, NV16, FILTER>, <CAMERA, SEMI, SHIFT, FILTER> (P210, P216, I210), <CAMERA, FILTER> at 8 and at 16 bits
KERNELS = ["framecam_422_kernelILi%dELb%dELi%dE" % (c, nv, f) for c in (0, 1) for nv in (0, 1) for f in (0, 1)]
KERNELS += ["framecam_422_16_kernelILi%dELb%dELi%dELi%dE" % (c, semi, shift, f) for c in (0, 1) for semi, shift in ((1, 6), (1, 0), (0, 0))
            for f in (0, 1)]
KERNELS += ["framecam_444_kernelILi%dELi%dE" % (c, f) for c in (0, 1) for f in (0, 1)]
KERNELS += ["framecam_444_16_kernelILi%dELi%dE" % (c, f) for c in (0, 1) for f in (0, 1)]


def test_public_header_is_c99(tmp_path):
    src = tmp_path / "zoomyuv.c"
    src.write_text('#include "rssync_zoomyuv.h"\n'
                   "int use(rssync_problem* p, const rssync_color_image* a, const rssync_color_image* b, const double* t, const rssync_lens* l,\n"
                   "        double* z, uint32_t* s) {\n"
                   "    rssync_color_params q = {0};\n"
                   "    return rssync_zoomyuv_fit(p, RSSYNC_YUV_P210, 4, 4, l, 4, 4, t, 1, 0.0, 0, &q, 1.0, 1.5, 0, z, s) == RSSYNC_ZOOM_CLEAR\n"
                   "        ? rssync_zoomyuv_stabilize(p, RSSYNC_YUV_NV16, a, 1, 4, 4, t, l, 0.0, 0, &q, b, 4, 4, 0, z) : -1;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o",
                    str(tmp_path / "zoomyuv.o"), str(src)], check=True)


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


def test_declared_exported_and_bound_functions_are_the_two(built):
    import rssync_amd
    from rssync_amd import zoomyuv
    text = open(os.path.join(ROOT, "include", "rssync_zoomyuv.h")).read()
    declared = set(re.findall(r"\b(rssync_zoomyuv_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == FUNCTIONS
    nm = subprocess.check_output(["nm", "-D", "--defined-only", rssync_amd.library_path()], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {e for e in exported if e.startswith("rssync_zoomyuv")} == FUNCTIONS
    assert "rship_zoomyuv_frames" in exported
    assert {name for name in zoomyuv.SIGNATURES if name.startswith("rssync_zoomyuv")} == FUNCTIONS
    zoomyuv.library()                   # binds every signature: a missing symbol raises
    for name in ("stabilize_yuv_zoomed", "stabilize_yuv_zoomed_budget", "fit_zoom_yuv", "dynamic_zoom_yuv"):
        assert callable(getattr(rssync_amd.SyncProblem, name)) and callable(getattr(zoomyuv, name))


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
        if "framecam_" in name:
            found[name] = {k: int(re.search(r"\.%s:\s+(\S+)" % k, block).group(1))
                           for k in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count",
                                     "sgpr_spill_count")}
    assert len(KERNELS) == 28
    for want in KERNELS:
        hit = [n for n in found if want in n]
        assert len(hit) == 1, (want, sorted(found))
        print(want, found[hit[0]])
    assert len(found) == len(KERNELS), sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert "FramecamArgs" in name
        # the names by which the tests of the other kernel families count theirs
        for other in ("zoom", "percam_", "bicubic", "limit_", "color_", "color16_", "stabilize", "rectify"):
            assert other not in name, (other, name)
        assert "infill" not in name.lower() and "donor" not in name.lower()
        assert not re.search(r"yuv4(22|44)(_16)?_kernel", name)


# ---- the fit's procedure in numpy -----------------------------------------------------------------------------------------
FIT_STEPS = 16      # at 10 or 12 steps the two planes' fits differ by at most a step: a test of the maximum shows nothing


def chroma_borders(site, targets=None):
    """step 2 of the header's procedure for case A: the 4:2:2 chroma plane as a camera of its own -- the chroma lens, the size
    (width / 2) x height, the frame times themselves, the chroma output camera at zoom 1 -- against the frame's target (the
    path at T with the lens's readout time, which the chroma lens keeps)"""
    s, c = rr.scene(), zr.CASES["A"]
    assert c["out_size"] is None
    lens_c = yr.chroma_lens422(s["lens"], site)
    cam_c = yr.chroma_camera422(s["lens"], rr.ROWS, rr.COLS, rr.ROWS, rr.COLS, site)
    from rssync_amd import synth
    return [zr.frame_border(s["gyro"], lens_c, rr.ROWS, rr.COLS // 2, t, synth.D_TRUE, target=None if targets is None else targets[f],
                            sigma=zr.SIGMA, out_size=(rr.COLS // 2, rr.ROWS), camera=c["camera"], cam=cam_c)
            for f, t in enumerate(zr.TIMES)]


def test_numpy_statement_of_the_fit_and_which_plane_sets_each_zoom():
    """case A at 16 steps, CENTER siting, the path's targets: the chroma plane sets the zoom of frames 0 .. 4 (by 6 .. 11
    steps of (hi - lo) / 2^16) and the luma plane that of frames 5 .. 8 (by 3 .. 20 steps); with LEFT siting the chroma plane
    sets frames 0 .. 4 and frames 5 .. 8 tie"""
    c = zr.CASES["A"]
    assert c["camera"] == sr.LENS and (c["lo"], c["hi"]) == (1.0, 1.5) and len(zr.TIMES) == 9
    step = (c["hi"] - c["lo"]) / 2 ** FIT_STEPS
    zl, sl = zr.fit64(zr.borders("A"), c["lo"], c["hi"], steps=FIT_STEPS)
    assert not sl.any()
    for site in (yr.CENTER, yr.LEFT):
        zc, sc = zr.fit64(chroma_borders(site), c["lo"], c["hi"], steps=FIT_STEPS)
        assert not sc.any()
        by = np.rint((zc - zl) / step).astype(int)
        print("site", site, "luma", zl.tolist(), "chroma", zc.tolist(), "chroma - luma in steps", by.tolist())
        np.testing.assert_array_equal((zc - zl) / step, by)         # (both are multiples of a step above lo)
        if site == yr.CENTER:
            assert (by[:5] >= 6).all() and (by[:5] <= 11).all(), by
            assert (by[5:] <= -3).all() and (by[5:] >= -20).all(), by
        else:
            assert (by[:5] > 0).all() and (by[5:] == 0).all(), by
        fitted = np.maximum(zl, zc)
        assert (fitted[:5] == zc[:5]).all() and (fitted[5:] == zl[5:]).all()
