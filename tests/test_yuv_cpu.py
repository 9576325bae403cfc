"""The 4:2:2 and 4:4:4 formats without a GPU (include/rssync_yuv.h): the new functions of csrc/color_math.hpp compiled for
the CPU against the numpy restatement (tests/yuv_reference.py), the chroma camera against the luma camera it must agree
with, the restatement against global-shutter renders of the 4:2:2 chroma planes, the float32 restatement against the
float64 one (where the device tolerance comes from), the header, and what the built library exports and holds."""
import os
import re
import subprocess

import numpy as np
import pytest

import color_reference as cr
import rectify_reference as rr
import stabilize_reference as sr
import yuv_reference as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
SITES = [yr.CENTER, yr.LEFT]


@pytest.fixture(scope="module")
def math_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("yuv") / "yuv_math_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpu_device", "yuv_math_check.cpp")],
                   check=True)
    return exe


@pytest.mark.parametrize("site", SITES)
def test_host_formulas_are_the_restatements_bit_for_bit(site, math_check):
    """csrc/color_math.hpp compiled for the CPU: the 4:2:2 offset, camera and frame time are the restatement's to the bit on a
    grid of cameras (the input lenses and the output cameras after scaling and zoom), and the 4:2:0 camera beside them is
    still cr.chroma_lens's"""
    t = float(rr.scene()["times"][1])
    cams = []
    for lens in yr.lens_grid():
        rows, cols = int(round(2 * lens[4])), int(round(2 * lens[3]))
        cams.append(tuple(lens[1:5]))
        for zoom in (0.8, 1.0, 1.3):
            cams.append(sr.out_camera(lens, rows, cols, 131, 198, zoom))
    assert len(cams) == 24
    for cam in cams:
        out = subprocess.run([math_check, str(site)] + [repr(float(v)) for v in cam] + [repr(t)], check=True, capture_output=True,
                             text=True).stdout.splitlines()
        fields = {line.split()[0]: [float.fromhex(v) for v in line.split()[1:]] for line in out}
        lens = (0.0,) + tuple(cam) + (0.0,) * 4
        assert fields["offset"] == [yr.OFFSET[site]]
        assert fields["camera"] == list(yr.chroma_lens422(lens, site)[1:5]), cam
        assert fields["time"] == [t]
        assert fields["camera420"] == list(cr.chroma_lens(lens, site)[1:5]), cam


@pytest.mark.parametrize("site", SITES)
def test_chroma_sample_and_its_luma_position_have_one_ray(site):
    """chroma sample (cu, cv) through the chroma lens and luma position (2 cu + ox, cv) through the lens: halving fx and
    cx - ox is exact in binary, so the two rays agree to the last bit where nothing underflows -- measured 0, bound 1e-15"""
    worst = max(yr.ray_agreement(lens, site) for lens in yr.lens_grid())
    print("site %d: the rays differ by at most %.3g" % (site, worst))
    assert worst <= yr.RAY_AGREEMENT


@pytest.mark.parametrize("site", SITES)
def test_chroma_map_agrees_with_the_luma_map_at_the_samples_luma_position(site):
    """the chroma map x (2, 1) + (ox, 0) is the luma map at (2 cu + ox, cv): one camera and one row table, so what remains
    is the rounding of the iteration -- below 1e-9 luma px on inside samples"""
    from rssync_amd import synth
    s = rr.scene()
    ox = yr.OFFSET[site]
    for out_size in (None, (198, 131)):
        oc, orows = (rr.COLS, rr.ROWS) if out_size is None else out_size
        px = sr.grid(orows, oc // 2) * np.array([2.0, 1.0]) + np.array([ox, 0.0])
        for t in s["times"][:2]:
            args = (s["gyro"], s["lens"], rr.ROWS, rr.COLS, t, synth.D_TRUE)
            chroma = yr.chroma_map64(*args, site, sigma=sr.SIGMA, out_size=out_size)
            luma = sr.map64(*args, sigma=sr.SIGMA, out_size=out_size, px=px)
            ok = sr.inside(chroma, yr.C_ROWS, yr.C_COLS)
            diff = np.abs(chroma * np.array([2.0, 1.0]) + np.array([ox, 0.0]) - luma)[ok].max()
            print("site %d out %s t %.3f: %.3g luma px" % (site, out_size, t, diff))
            assert ok.mean() > 0.9 and diff < 1e-9


def test_the_422_row_table_is_the_lumas():
    """the chroma lens keeps ro, the plane keeps the rows and the frame keeps its time: the same table, bit for bit"""
    from rssync_amd import synth
    s = rr.scene()
    q = sr.path(sr.SIGMA)[1]
    luma = sr.row_table(s["gyro"], s["lens"], rr.ROWS, s["times"][1], synth.D_TRUE, q)
    for site in SITES:
        chroma = sr.row_table(s["gyro"], yr.chroma_lens422(s["lens"], site), yr.C_ROWS, s["times"][1], synth.D_TRUE, q)
        assert chroma.shape == (rr.ROWS + 1, 3, 3)
        np.testing.assert_array_equal(chroma.view(np.uint64), luma.view(np.uint64))


@pytest.mark.parametrize("site", SITES)
def test_reference_renders_the_chroma_truth_at_the_smoothed_path(site):
    errors = yr.chroma_errors(site)
    for p, name in enumerate("UV"):
        for k in range(rr.N_FRAMES):
            err, raw = errors[p][k]
            print("site %d %s frame %d: stabilised %.4f raw %.1f" % (site, name, rr.F0 + k, err, raw))
            assert abs(err - yr.REFERENCE_ERROR[site][p][k]) <= 5e-4 and abs(raw - yr.RAW_ERROR[site][p][k]) <= 0.05, (p, k, err, raw)
            assert err <= rr.RATIO * raw


@pytest.mark.parametrize("camera", [sr.LENS, sr.PINHOLE])
def test_float32_restatement_of_the_chroma_map_against_float64(camera):
    tol = yr.device_tolerance(camera)
    print("camera %d: device tolerance %.3g chroma px" % (camera, tol))
    assert 0 < tol / 4 <= yr.MAP_SPREAD and tol * 255 < 0.5
    for site in SITES:
        for out_size in (None, (198, 131)):
            spread = yr.map_spread(camera, site, out_size)
            print("  site %d out %s: float32 %.3g chroma px" % (site, out_size, spread))
            assert 0 < spread <= yr.MAP_SPREAD


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


def test_header_compiles_as_c99_and_declares_two_functions(tmp_path):
    text = open(os.path.join(ROOT, "include", "rssync_yuv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(rssync_\w+)\s*\(", code)) == {"rssync_yuv_stabilize", "rssync_yuv_map"}
    for word in ("zoom per frame", "infill", "YUY2", "UYVY", "v210", "beyond I410"):
        assert word in text, word
    src = tmp_path / "use.c"
    src.write_text('#include "rssync_yuv.h"\n'
                   "int use(rssync_problem* p, const rssync_color_image* a, const rssync_color_image* b, const double* t, const rssync_lens* l, float* m) {\n"
                   "    rssync_color_params q = {0};\n"
                   "    return RSSYNC_YUV_I422 == 32 && RSSYNC_YUV_NV16 == 33 && RSSYNC_YUV_I444 == 34 && RSSYNC_YUV_I210 == 48 && RSSYNC_YUV_P210 == 49\n"
                   "            && RSSYNC_YUV_P216 == 50 && RSSYNC_YUV_I410 == 51\n"
                   "        ? rssync_yuv_stabilize(p, RSSYNC_YUV_P210, a, 1, 4, 3, t, l, 0.0, 0, &q, b, 4, 3, 0)\n"
                   "          + rssync_yuv_map(p, RSSYNC_YUV_NV16, 1, 4, 3, l, 4, 3, t[0], 0.0, 0, &q, m) : -1;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-missing-field-initializers", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "use.o")], check=True)


def test_library_exports_the_entries_and_holds_the_kernels(built, tmp_path):
    import rssync_amd
    from rssync_amd import color, yuv
    assert (yuv.I422, yuv.NV16, yuv.I444, yuv.I210, yuv.P210, yuv.P216, yuv.I410) == (32, 33, 34, 48, 49, 50, 51)
    lib = rssync_amd.library_path()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {e for e in exported if e.startswith("rssync_yuv")} == {"rssync_yuv_stabilize", "rssync_yuv_map"}
    assert {e for e in exported if e.startswith("rship_yuv")} == {"rship_yuv_frames", "rship_yuv_map"}
    assert yuv.SIGNATURES["rssync_yuv_stabilize"] == color.SIGNATURES["rssync_color_stabilize"]
    assert yuv.SIGNATURES["rssync_yuv_map"] == color.SIGNATURES["rssync_color_map"]
    yuv.library()                   # binds every signature: a missing symbol raises
    for name in ("stabilize_yuv", "yuv_map", "stabilize_yuv_budget"):
        assert callable(getattr(rssync_amd.SyncProblem, name)) and callable(getattr(yuv, name))
    for fmt, sib in yuv.SIBLING.items():
        assert yuv.plane_shapes(fmt, 3, 7, 12) == yuv.plane_shapes(sib, 3, 7, 12)
    assert yuv.plane_shapes(yuv.I422, 3, 7, 12) == [(3, 7, 12), (3, 7, 6), (3, 7, 6)]
    assert yuv.plane_shapes(yuv.NV16, 3, 7, 12) == [(3, 7, 12), (3, 7, 6, 2)]
    assert yuv.plane_shapes(yuv.I444, 3, 7, 11) == [(3, 7, 11)] * 3
    # the code object: the 28 instantiations are there, each once, without a private segment or spills
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if re.search(r"yuv4(22|44)(_16)?_kernel", name):
            found[name] = sum(int(re.search(r"\.%s:\s+(\S+)" % key, block).group(1))
                              for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"))
    want = ["yuv422_kernelILi%dELb%dELi%dEE" % (c, nv, f) for c in (0, 1) for nv in (0, 1) for f in (0, 1)]
    want += ["yuv422_16_kernelILi%dELb%dELi%dELi%dEE" % (c, semi, sh, f) for c in (0, 1) for semi, sh in ((1, 6), (1, 0), (0, 0)) for f in (0, 1)]
    want += ["yuv444_kernelILi%dELi%dEE" % (c, f) for c in (0, 1) for f in (0, 1)]
    want += ["yuv444_16_kernelILi%dELi%dEE" % (c, f) for c in (0, 1) for f in (0, 1)]
    assert len(want) == 28
    for w in want:
        assert len([n for n in found if w in n]) == 1, (w, sorted(found))
    assert len(found) == 28 and not any(found.values()), found
