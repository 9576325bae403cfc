"""The 16-bit colour front without a GPU (include/rssync_color16.h): its numpy restatement (tests/color16_reference.py)
against the 8-bit one it widens, the sampler's arithmetic in csrc/color_math.hpp compiled for the CPU, the header, and what
the built library exports and holds."""
import os
import re
import subprocess

import numpy as np
import pytest

import color16_reference as c16
import color_reference as cr
import rectify_reference as rr
import stabilize_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_restatement_on_8_bit_values_is_the_8_bit_restatement_widened():
    """uint16 data whose values are the scene's 8-bit values: the same taps, weights and float32 operations, so the same
    numbers -- on the scene's three frames along the reference maps (LENS, same size: thousands of filled samples)"""
    s = cr.scene()
    for k in range(rr.N_FRAMES):
        m = sr.reference_maps()[k]
        want, want_n = sr.sample(s["y"][k], m, fill=9)
        got, got_n = c16.sample16(s["y"][k].astype(np.uint16), m, fill=9)
        assert got.dtype == np.uint16 and got_n == want_n > 0
        np.testing.assert_array_equal(got, want.astype(np.uint16))
        mc = cr.reference_maps()[k]
        want, want_n = cr.sample_pairs(s["uv"][k], mc, fill=(3, 4))
        got, got_n = c16.sample_pairs16(s["uv"][k].astype(np.uint16), mc, fill=(3, 4))
        assert got.dtype == np.uint16 and got_n == want_n > 0
        np.testing.assert_array_equal(got, want.astype(np.uint16))


def test_pack_and_unpack_are_the_shift_of_the_container():
    rng = np.random.default_rng(5)
    v10 = rng.integers(0, 1024, size=(7, 9), dtype=np.uint16)
    v16 = rng.integers(0, 65536, size=(7, 9), dtype=np.uint16)
    (w,) = c16.pack(c16.P010, (v10,))
    assert w.dtype == np.uint16
    np.testing.assert_array_equal(w, v10 << 6)
    np.testing.assert_array_equal(c16.unpack(c16.P010, (w | rng.integers(0, 64, size=w.shape, dtype=np.uint16),))[0], v10)
    for fmt, v in ((c16.GRAY16, v16), (c16.P016, v16), (c16.I010, v10)):
        np.testing.assert_array_equal(c16.pack(fmt, (v,))[0], v)
        np.testing.assert_array_equal(c16.unpack(fmt, (v,))[0], v)


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_sampler_arithmetic_compiled_for_the_cpu(tmp_path):
    """csrc/color_math.hpp with g++ -ffp-contract=off: color_blend16 is color_blend on taps <= 255, its result stays within
    the range of its four taps at the extremes of 10 and 16 bits (weights 0, 1 and the float below 1 included), and P010's
    container is >> 6 and << 6"""
    exe = str(tmp_path / "color16_math_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpu_device", "color16_math_check.cpp")],
                   check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    fields = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out}
    print(fields)
    assert fields["blend8"][0] > 1000000 and fields["blend8"][1] == 0
    assert fields["range"][0] > 1000000 and fields["range"][1] == 0
    assert fields["p010"] == [65536, 0]


# 3 and 4 ---------------------------------------------------------------------------------------------------------------
def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


def test_header_compiles_as_c99_and_declares_one_function(tmp_path):
    text = open(os.path.join(ROOT, "include", "rssync_color16.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(rssync_\w+)\s*\(", code)) == {"rssync_color16_stabilize"}
    src = tmp_path / "use.c"
    src.write_text('#include "rssync_color16.h"\n'
                   "int use(rssync_problem* p, const rssync_color_image* a, const rssync_color_image* b, const double* t, const rssync_lens* l) {\n"
                   "    rssync_color_params q = {0};\n"
                   "    return RSSYNC_COLOR16_GRAY16 == 16 && RSSYNC_COLOR16_P010 == 17 && RSSYNC_COLOR16_P016 == 18 && RSSYNC_COLOR16_I010 == 19\n"
                   "        ? rssync_color16_stabilize(p, RSSYNC_COLOR16_P010, a, 1, 4, 4, t, l, 0.0, 0, &q, b, 4, 4, 0) : -1;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-Wno-missing-field-initializers", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "use.o")], check=True)


def test_library_exports_the_16_bit_entry_and_holds_its_kernels(built, tmp_path):
    import rssync_amd
    from rssync_amd import color
    assert (color.GRAY16, color.P010, color.P016, color.I010) == (16, 17, 18, 19)
    lib = rssync_amd.library_path()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {e for e in exported if e.startswith("rssync_color16")} == {"rssync_color16_stabilize"}
    assert {name for name in color.SIGNATURES if name.startswith("rssync_color16")} == {"rssync_color16_stabilize"}
    assert color.SIGNATURES["rssync_color16_stabilize"] == color.SIGNATURES["rssync_color_stabilize"]
    color.library()                 # binds every signature: a missing symbol raises
    for fmt, sib in ((color.GRAY16, color.GRAY8), (color.P010, color.NV12), (color.P016, color.NV12), (color.I010, color.I420)):
        assert color.plane_shapes(fmt, 3, 8, 12) == color.plane_shapes(sib, 3, 8, 12)
    # the code object: every 16-bit kernel is there, for both cameras, and has no private segment
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    private = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "color16_" in name:
            private[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\S+)", block).group(1))
    want = ["color16_gray_kernelILi%dE" % c for c in (0, 1)]
    want += ["color16_yuv_kernelILi%dELb%dELi%dE" % (c, semi, shift) for c in (0, 1) for semi, shift in ((1, 6), (1, 0), (0, 0))]
    for w in want:
        assert [n for n in private if w in n], (w, sorted(private))
    assert len(private) == len(want) and not any(private.values()), private
