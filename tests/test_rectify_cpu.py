"""The rectifier without a GPU: its numpy restatement (tests/rectify_reference.py) against the synthetic video's ground
truth, the float32 restatement against the float64 one (where the device tolerance comes from), the forward points as
the map's inverse, and what the built library exports."""
import os
import re
import subprocess

import numpy as np
import pytest

import rectify_reference as rr
from rectify_reference import RATIO, REFERENCE_ERROR, UNRECTIFIED_ERROR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
MAP_SPREAD = 1.6e-4  # px: the float32 restatement against the float64 one at 380 x 676, as first measured


def test_reference_removes_the_skew_of_the_synthetic_video():
    from rssync_amd import synth  # noqa: F401
    s, maps = rr.scene(), rr.reference_maps()
    for k in range(rr.N_FRAMES):
        ok = rr.inside(maps[k])
        img, n_out = rr.sample(s["frames"][k], maps[k])
        err = rr.grey_error(img, s["truth"][k], ok)
        raw = rr.grey_error(s["frames"][k], s["truth"][k], ok)
        print("frame %d: rectified %.4f unrectified %.4f outside %.4f" % (rr.F0 + k, err, raw, n_out / ok.size))
        assert abs(err - REFERENCE_ERROR[k]) <= 5e-4 and abs(raw - UNRECTIFIED_ERROR[k]) <= 5e-4, (k, err, raw)
        assert n_out == (~ok).sum() and 0.002 <= n_out / ok.size <= 0.007
        if k != 1:
            assert err <= RATIO * raw, (k, err, raw)


def test_float32_restatement_against_float64():
    """the spread the device tolerance is four times of; the third iteration moves the map by ~2e-5 px, a fourth by
    nothing that matters"""
    from rssync_amd import synth
    s = rr.scene()
    tol = rr.device_tolerance()
    print("float32 against float64 at %d x %d: %.3g px; device tolerance %.3g px" % (rr.ROWS, rr.COLS, tol / 4, tol))
    assert 0 < tol / 4 <= MAP_SPREAD
    assert tol * 255 < 0.5      # (what "at most one grey level between device and reference" rests on)
    args = (s["gyro"], s["lens"], rr.ROWS, rr.COLS, s["times"][0], synth.D_TRUE)
    m2, m3, m4 = (rr.map64(*args, iterations=i) for i in (2, 3, 4))
    assert 1e-6 < np.abs(m3 - m2).max() < 1e-4 and np.abs(m4 - m3).max() < 1e-6


@pytest.mark.parametrize("ref_row", [None, 0, rr.ROWS])
def test_forward_points_undo_the_map(ref_row):
    from rssync_amd import synth
    s = rr.scene()
    m = rr.map64(s["gyro"], s["lens"], rr.ROWS, rr.COLS, s["times"][0], synth.D_TRUE, ref_row=ref_row)
    back = rr.forward_points(s["gyro"], s["lens"], rr.ROWS, s["times"][0], synth.D_TRUE, m, ref_row=ref_row)
    ys, xs = np.mgrid[0:rr.ROWS, 0:rr.COLS]
    ok = rr.inside(m)    # (outside the frame the map clamps the row it takes the orientation of; the points do not)
    assert ok.mean() > 0.95
    assert np.abs(back - np.stack([xs, ys], axis=-1))[ok].max() <= rr.device_tolerance()


def test_sampler_restatement_at_pixel_centres_and_edges():
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, size=(9, 7), dtype=np.uint8)
    ys, xs = np.mgrid[0:9, 0:7]
    ident = np.stack([xs, ys], axis=-1).astype(np.float32)
    out, n = rr.sample(frame, ident)
    np.testing.assert_array_equal(out, frame)
    assert n == 0
    m = ident.copy()
    m[0, 0] = (-1e-3, 0)
    m[1, 1] = (6.001, 3)
    m[2, 2] = (np.nan, 1)
    m[3, 3] = (2.5, 4.5)
    out, n = rr.sample(frame, m, fill=9)
    assert n == 3 and out[0, 0] == 9 and out[1, 1] == 9 and out[2, 2] == 9
    assert out[3, 3] == np.rint(frame[4:6, 2:4].astype(np.float64).mean())


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


def test_library_exports_the_rectifier_and_its_kernels_use_no_scratch(built, tmp_path):
    import rssync_amd
    from rssync_amd import rectify
    lib = rssync_amd.library_path()
    text = open(os.path.join(ROOT, "include", "rssync_rectify.h")).read()
    declared = set(re.findall(r"\b(rssync_rectify_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == {"rssync_rectify_map", "rssync_rectify_frames", "rssync_rectify_points"}
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not (declared - exported), sorted(declared - exported)
    assert declared <= set(rectify.SIGNATURES)
    rectify.library()                   # binds every signature: a missing symbol raises
    # the code object: every rectifier kernel is there and has no private segment
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    private = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "rectify" in name:
            private[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\S+)", block).group(1))
    for want in ("rectify_rays_kernel", "rectify_rows_kernel", "rectify_kernelILb0", "rectify_kernelILb1", "rectify_points_kernel"):
        assert [n for n in private if want in n], (want, sorted(private))
    assert not any(private.values()), private
