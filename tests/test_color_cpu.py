"""The colour front without a GPU: its numpy restatement (tests/color_reference.py) against global-shutter renders of the
chroma planes at the smoothed path's orientations, the chroma map against the luma map it must agree with, the float32
restatement against the float64 one (where the device tolerance comes from), and what the built library exports."""
import os
import re
import subprocess

import numpy as np
import pytest

import color_reference as cr
import rectify_reference as rr
import stabilize_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
MAP_SPREAD = 7e-5   # chroma px: the float32 restatement against the float64 one, the largest over cameras and sitings as first measured
SITES = [cr.CENTER, cr.LEFT]


@pytest.mark.parametrize("site", SITES)
def test_reference_renders_the_chroma_truth_at_the_smoothed_path(site):
    errors = cr.chroma_errors(site)
    for p, name in enumerate("UV"):
        for k in range(rr.N_FRAMES):
            err, raw = errors[p][k]
            print("site %d %s frame %d: stabilised %.4f raw %.1f" % (site, name, rr.F0 + k, err, raw))
            assert abs(err - cr.REFERENCE_ERROR[site][p][k]) <= 5e-4 and abs(raw - cr.RAW_ERROR[site][p][k]) <= 0.05, (p, k, err, raw)
            assert err <= rr.RATIO * raw


def test_the_render_with_another_texture_keeps_the_camera_path():
    """texture_seed changes what the walls carry, nothing else: the default is the old render, and U differs from Y"""
    from rssync_amd import synth_video as sv
    s = rr.scene()
    kw = dict(lens=rr.scaled_lens(38, 68), rows=38, cols=68, seed=rr.SEED)
    a, ta = sv.render(s["gyro"], rr.F0, rr.F0 + 1, **kw)
    b, tb = sv.render(s["gyro"], rr.F0, rr.F0 + 1, texture_seed=rr.SEED, **kw)
    c, _ = sv.render(s["gyro"], rr.F0, rr.F0 + 1, texture_seed=cr.U_SEED, **kw)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ta, tb)
    assert np.abs(a.astype(int) - c.astype(int)).mean() > 10
    col = cr.scene()
    assert np.abs(col["u"].astype(int) - col["v"].astype(int)).mean() > 10


@pytest.mark.parametrize("site", SITES)
def test_chroma_map_agrees_with_the_luma_map_at_the_samples_luma_position(site):
    """the chroma map x 2 + (ox, oy) is the luma map at (2 cu + ox, 2 cv + oy): the two cameras are one camera, and the two
    row tables one rotation, up to where the chroma table's knots lie -- below 1e-4 luma px on inside samples"""
    from rssync_amd import synth
    s = rr.scene()
    ox, oy = cr.OFFSET[site]
    for out_size in (None, (320, 200)):
        oc, orows = (rr.COLS, rr.ROWS) if out_size is None else out_size
        px = sr.grid(orows // 2, oc // 2) * 2.0 + np.array([ox, oy])
        for t in s["times"][:2]:
            args = (s["gyro"], s["lens"], rr.ROWS, rr.COLS, t, synth.D_TRUE)
            chroma = cr.chroma_map64(*args, site, sigma=sr.SIGMA, out_size=out_size)
            luma = sr.map64(*args, sigma=sr.SIGMA, out_size=out_size, px=px)
            ok = sr.inside(chroma, cr.C_ROWS, cr.C_COLS)
            diff = np.abs(chroma * 2.0 + np.array([ox, oy]) - luma)[ok].max()
            print("site %d out %s t %.3f: %.3g luma px" % (site, out_size, t, diff))
            assert ok.mean() > 0.9 and diff < 1e-4


@pytest.mark.parametrize("camera", [sr.LENS, sr.PINHOLE])
def test_float32_restatement_of_the_chroma_map_against_float64(camera):
    tol = cr.device_tolerance(camera)
    print("camera %d: device tolerance %.3g chroma px" % (camera, tol))
    assert 0 < tol / 4 <= MAP_SPREAD and tol * 255 < 0.5
    for site in SITES:
        for out_size in (None, (320, 200)):
            spread = cr.map_spread(camera, site, out_size)
            print("  site %d out %s: float32 %.3g chroma px" % (site, out_size, spread))
            assert 0 < spread <= MAP_SPREAD


def test_samplers_are_the_stabilisers_per_channel():
    s = cr.scene()
    m = cr.reference_maps()[0]
    uv, n = cr.sample_pairs(s["uv"][0], m, fill=(3, 4))
    u, nu = sr.sample(s["u"][0], m, fill=3)
    v, _ = sr.sample(s["v"][0], m, fill=4)
    np.testing.assert_array_equal(uv[..., 0], u)
    np.testing.assert_array_equal(uv[..., 1], v)
    assert n == nu > 0
    rgba = np.stack([s["u"][0], s["v"][0], s["u"][0][::-1], s["v"][0][:, ::-1]], axis=-1)
    got, n4 = cr.sample_rgba(rgba, m)
    np.testing.assert_array_equal(got[..., 1], sr.sample(s["v"][0], m)[0])
    assert n4 == n and (got[..., 3][~sr.inside(m, cr.C_ROWS, cr.C_COLS)] == 255).all()


@pytest.mark.parametrize("site", SITES)
def test_host_formulas_and_the_sampler_taken_apart(site, tmp_path):
    """csrc/color_math.hpp compiled for the CPU: the chroma camera and frame time the host forms are the restatement's to
    the bit, and color_taps + color_blend give rect_sample's byte at every position of a sweep"""
    s = rr.scene()
    exe = str(tmp_path / "color_math_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "cpu_device", "color_math_check.cpp")],
                   check=True)
    lens, t = s["lens"], float(s["times"][1])
    out = subprocess.run([exe, str(site)] + [repr(float(v)) for v in lens[:5]] + [str(rr.ROWS), repr(t)], check=True, capture_output=True,
                         text=True).stdout.splitlines()
    fields = {line.split()[0]: line.split()[1:] for line in out}
    assert [float.fromhex(v) for v in fields["camera"]] == list(cr.chroma_lens(lens, site)[1:5])
    assert float.fromhex(fields["time"][0]) == cr.chroma_time(t, lens, rr.ROWS, site)
    assert t + float.fromhex(fields["offset"][0]) == cr.chroma_time(t, lens, rr.ROWS, site)      # (what the launcher adds to T)
    assert int(fields["sampler"][0]) > 6000 and fields["sampler"][2] == "0", fields["sampler"]


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


def test_library_exports_the_colour_front_and_holds_its_kernels(built, tmp_path):
    import rssync_amd
    from rssync_amd import color
    lib = rssync_amd.library_path()
    text = open(os.path.join(ROOT, "include", "rssync_color.h")).read()
    declared = set(re.findall(r"\b(rssync_color_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == {"rssync_color_stabilize", "rssync_color_map"}
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert declared == {e for e in exported if e.startswith("rssync_color_")}
    assert declared == {name for name in color.SIGNATURES if name.startswith("rssync_color_")}
    color.library()                 # binds every signature: a missing symbol raises
    for name in ("stabilize_color", "color_map"):
        assert callable(getattr(rssync_amd.SyncProblem, name)) and callable(getattr(color, name))
    # the code object: every colour kernel is there and has no private segment
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    private = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "color_" in name:
            private[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\S+)", block).group(1))
    for want in ("color_rows_kernel", "color_yuv_kernelILi0ELb0", "color_yuv_kernelILi0ELb1", "color_yuv_kernelILi1ELb0",
                 "color_yuv_kernelILi1ELb1", "color_rgba_kernelILi0", "color_rgba_kernelILi1"):
        assert [n for n in private if want in n], (want, sorted(private))
    assert not any(private.values()), private
