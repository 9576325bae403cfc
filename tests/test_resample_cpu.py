"""The bicubic sampler without a GPU: the public struct's layout, csrc/resample_math.hpp compiled for the CPU against the
numpy restatement (tests/resample_reference.py) byte for byte, the restatement's own properties, what the sharper kernel
buys on noise and on a band-limited signal, and the bicubic kernels in the built library's code object."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import color16_reference as c16
import rectify_reference as rr
import resample_reference as q
import stabilize_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
CHECK = os.path.join(ROOT, "tests", "cpu_device", "resample_math_check.cpp")
F = np.float32


def test_struct_layout_in_python():
    from rssync_amd import color, stabilize
    assert ctypes.sizeof(stabilize.StabilizeParams) == 64
    assert stabilize.StabilizeParams.filter.offset == 60
    assert color.ColorParams.chroma_site.offset == 64
    assert ctypes.sizeof(stabilize._Cfg) == 176 and stabilize._Cfg.filter.offset == 172
    assert (stabilize.FILTER_BILINEAR, stabilize.FILTER_BICUBIC) == (0, 1)
    prm = stabilize.params()
    assert prm.filter == 0 and stabilize.params(filter=stabilize.FILTER_BICUBIC).filter == 1
    assert color.params(filter=stabilize.FILTER_BICUBIC).stab.filter == 1 and color.params().stab.filter == 0


def test_struct_layout_in_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rssync_stabilize.h"\n#include "rssync_color.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %d\\n", sizeof(rssync_stabilize_params), offsetof(rssync_stabilize_params, filter),\n'
                   'offsetof(rssync_color_params, chroma_site), RSSYNC_FILTER_BILINEAR, RSSYNC_FILTER_BICUBIC); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    assert subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split() == ["64", "60", "64", "0", "1"]


def _run_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, CHECK], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def header_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_check")
    plain = _run_check(d, "plain", [])
    # host code in a stand-alone program: the sanitizers' runtimes are linked in, nothing is preloaded
    checked = _run_check(d, "sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    return plain, checked


def test_header_gives_the_restatements_bytes(header_output):
    plain, checked = header_output
    assert plain == checked, "the sanitized build printed something else"
    planes, got = {}, {}
    for line in plain.splitlines():
        f = line.split()
        if f[0] == "plane":
            planes[f[1]] = np.array([int(v) for v in f[2:]], np.uint16).reshape(7, 9)
        elif f[0] == "s":
            got.setdefault(f[1], []).append((float.fromhex(f[2]), float.fromhex(f[3]), int(f[4])))
    assert sorted(planes) == ["i010", "p010", "u16", "u8"]
    fmt = {"i010": c16.I010, "p010": c16.P010, "u16": c16.GRAY16}
    for tag, plane in planes.items():
        pts = np.array(got[tag], np.float64)
        m = pts[:, None, :2].astype(F)
        assert len(pts) > 1000 and sr.inside(m, 7, 9).all()
        xs, ys = set(pts[:, 0]), set(pts[:, 1])
        assert {0.0, 8.0, float(F(8) - F(1e-3)), float(F(1e-3))} <= xs and {0.0, 6.0, float(F(6) - F(1e-3))} <= ys   # edges, and near them
        assert set(range(9)) <= xs and set(range(7)) <= ys                                               # every integer position
        cl = {}
        if tag == "u8":
            want, n = q.sample_bicubic(plane.astype(np.uint8), m, clamped=cl)
        else:
            want, n = q.sample_bicubic16(fmt[tag], plane, m, clamped=cl)
        assert n == 0 and cl["low"] > 0 and cl["high"] > 0, cl                                           # the clamp works at both ends
        np.testing.assert_array_equal(want[:, 0].astype(np.int64), pts[:, 2].astype(np.int64), err_msg=tag)
        if tag == "p010":
            assert (pts[:, 2].astype(np.int64) & 63 == 0).all() and (plane & 63).any()
    w = [[float.fromhex(v) for v in line.split()[1:]] for line in plain.splitlines() if line.startswith("weights")]
    assert len(w) == 7
    for t, *ws in w:
        assert ws == [float(v) for v in q.weights(F(t))], t
    assert w[0][1:] == [0.0, 1.0, 0.0, 0.0] and np.signbit(w[0][1]) and w[1][1:] == [0.0, 0.0, 1.0, 0.0]


def _identity_map(rows, cols, dx=0.0, dy=0.0):
    return (sr.grid(rows, cols) + np.array([dx, dy])).astype(F)


def test_integer_grid_reproduces_the_frame_and_constants_stay_constant():
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (23, 31), dtype=np.uint8)
    got, n = q.sample_bicubic(frame, _identity_map(23, 31))
    assert n == 0
    np.testing.assert_array_equal(got, frame)                       # edges and corners included
    wide = rng.integers(0, 65536, (23, 31), dtype=np.uint16)
    np.testing.assert_array_equal(q.sample_bicubic(wide, _identity_map(23, 31), vmax=65535)[0], wide)
    m = (rng.random((40, 50, 2)) * np.array([30.0, 22.0])).astype(F)   # fractional positions all over the plane
    for top, dtype in ((255, np.uint8), (1023, np.uint16), (65535, np.uint16)):
        const = np.full((23, 31), top, dtype)
        got, n = q.sample_bicubic(const, m, vmax=top)
        assert n == 0 and (got == top).all(), top


def test_weights_sum_to_one():
    """2.39e-7 as first measured over 100001 values of t, with a factor of two for another sweep density"""
    for n in (100001, 65537):
        w = q.weights(np.linspace(0, 1, n).astype(F))
        s = (w[0] + w[1]) + (w[2] + w[3])
        assert s.dtype == F
        err = float(np.abs(s.astype(np.float64) - 1).max())
        print("%d values of t: %.3g" % (n, err))
        assert err <= 5e-7


def test_bicubic_keeps_more_of_a_noise_frame():
    lin, cub, own, n_clamped, n_inside = q.noise_stds()
    print("noise %.1f: bilinear %.1f bicubic %.1f, %d of %d inside pixels clamp" % (own, lin, cub, n_clamped, n_inside))
    assert abs(lin - q.NOISE_STD[0]) <= 0.05 and abs(cub - q.NOISE_STD[1]) <= 0.05
    assert n_clamped > 0 and cub >= 1.15 * lin and cub < own


def test_scene_error_is_the_recorded_one_and_not_better_than_bilinear():
    errors = q.scene_errors()
    print(" / ".join("%.4f" % e for e in errors))
    for k in range(rr.N_FRAMES):
        assert abs(errors[k] - q.BICUBIC_ERROR[k]) <= 5e-4
        assert errors[k] > sr.REFERENCE_ERROR[k]          # said plainly in INTEGRATION.md: detail kept, not this figure
        assert errors[k] <= 0.25 * sr.RAW_ERROR[k]


def test_band_limited_signal_at_half_a_pixel():
    """a horizontal sinusoid of period 6 px sampled half a pixel off the grid: the kernels' gains there are 0.974 (bicubic)
    and 0.866 (bilinear), so the bicubic error is about a fifth of the bilinear one; asserted: at most half"""
    rows, cols = 16, 96
    x = np.arange(cols, dtype=np.float64)
    frame = np.broadcast_to(np.rint(128 + 100 * np.sin(2 * np.pi * x / 6)), (rows, cols)).astype(np.uint8)
    m = _identity_map(rows, cols, dx=0.5)
    truth = 128 + 100 * np.sin(2 * np.pi * (x + 0.5) / 6)
    keep = slice(4, cols - 5)
    lin = np.abs(sr.sample(frame, m)[0].astype(np.float64) - truth)[:, keep].mean()
    cub = np.abs(q.sample_bicubic(frame, m)[0].astype(np.float64) - truth)[:, keep].mean()
    print("bilinear %.3f bicubic %.3f ratio %.3f" % (lin, cub, cub / lin))
    assert cub <= 0.5 * lin


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


BICUBIC_KERNELS = (["stabilize_bicubic_kernelILi%dE" % c for c in (0, 1)] +
                   ["bicubic_yuv_kernelILi%dELb%dE" % (c, nv) for c in (0, 1) for nv in (0, 1)] +
                   ["bicubic_rgba_kernelILi%dE" % c for c in (0, 1)] +
                   ["bicubic16_gray_kernelILi%dE" % c for c in (0, 1)] +
                   ["bicubic16_yuv_kernelILi%dELb%dELi%dE" % (c, semi, sh) for c in (0, 1) for semi, sh in ((1, 6), (1, 0), (0, 0))])


def test_library_holds_every_bicubic_kernel_without_a_private_segment(built, tmp_path):
    import rssync_amd
    lib = rssync_amd.library_path()
    # no new symbol: the filter is a field
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {e for e in exported if e.startswith("rssync_stabilize_")} == {"rssync_stabilize_path", "rssync_stabilize_map", "rssync_stabilize_frames",
                                                                         "rssync_stabilize_coverage"}
    assert not [e for e in exported if "bicubic" in e or "filter" in e]
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "bicubic" in name:
            found[name] = {k: int(re.search(r"\.%s:\s+(\S+)" % k, block).group(1))
                           for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    for want in BICUBIC_KERNELS:
        hit = [n for n in found if want in n]
        assert len(hit) == 1, (want, sorted(found))
        print(want, found[hit[0]])
    assert len(found) == len(BICUBIC_KERNELS) == 16, sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
