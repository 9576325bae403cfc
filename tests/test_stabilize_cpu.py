"""The stabiliser without a GPU: its numpy restatement (tests/stabilize_reference.py) against the rectifier's and against
global-shutter renders at the smoothed path's orientations, the float32 restatement against the float64 one (where the
device tolerances come from), the border counts, and what the built library exports."""
import os
import re
import subprocess

import numpy as np
import pytest

import rectify_reference as rr
import stabilize_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
MAP_SPREAD = 1.6e-4  # px: the float32 restatement against the float64 one, the largest over cameras and sizes as first measured


def _args():
    from rssync_amd import synth
    s = rr.scene()
    return s, (s["gyro"], s["lens"], rr.ROWS, rr.COLS, s["times"][0], synth.D_TRUE)


def test_path_without_smoothing_is_the_centre_orientation():
    from rssync_amd import synth
    s = rr.scene()
    g, ro = s["gyro"], s["lens"][0]
    want = g.orientation(s["times"] + ro * 0.5 + synth.D_TRUE)
    np.testing.assert_array_equal(sr.path64(g, s["times"], ro, synth.D_TRUE, 0.0), want)
    # a short window stays close to it and is a unit quaternion; a long one clamps at both ends of the gyro and still is one
    for sigma, far in ((1e-3, 1e-4), (1.0, 2.0)):
        q = sr.path64(g, s["times"], ro, synth.D_TRUE, sigma)
        assert np.abs(np.linalg.norm(q, axis=-1) - 1).max() < 1e-14 and np.abs(q - want).max() < far


def test_map_at_the_rectifiers_target_is_the_rectifiers_map():
    s, args = _args()
    q_ref = s["gyro"].orientation(args[4] + s["lens"][0] * 0.5 + args[5])
    want = rr.map64(*args)
    np.testing.assert_array_equal(sr.map64(*args, sigma=0.0), want)         # (the path at sigma 0 IS q_ref, to the bit)
    np.testing.assert_array_equal(sr.map32(*args), rr.map32(*args))
    np.testing.assert_array_equal(sr.row_table(s["gyro"], s["lens"], rr.ROWS, args[4], args[5], q_ref),
                                  rr.row_table(s["gyro"], s["lens"], rr.ROWS, args[4], args[5]))
    # a caller's target is normalised once more, as the library does: q_ref moves by an ulp, the map by 1e-12 px
    assert np.abs(sr.map64(*args, target=q_ref) - want).max() < 1e-11
    assert np.abs(sr.map64(*args, target=-3.0 * q_ref) - want).max() < 1e-11


@pytest.mark.parametrize("camera", [sr.LENS, sr.PINHOLE])
def test_float32_restatement_against_float64(camera):
    """the spreads the device tolerances are four times of, over the output sizes of the device test and a larger one;
    the third iteration moves the map by less than 0.005 px, three more by nothing that matters"""
    s, args = _args()
    tol = sr.device_tolerance(camera)
    print("camera %d: float32 against float64 at %d x %d: %.3g px; device tolerance %.3g px" % (camera, rr.ROWS, rr.COLS, tol / 4, tol))
    assert 0 < tol / 4 <= MAP_SPREAD and tol * 255 < 0.5
    for out_size in ((rr.COLS, rr.ROWS), (320, 200), (854, 480), (29, 37)):
        kw = dict(sigma=sr.SIGMA, out_size=out_size, camera=camera)
        m2, m3, m6 = (sr.map64(*args, iterations=i, **kw) for i in (2, 3, 6))
        spread = np.abs(sr.map32(*args, **kw).astype(np.float64) - m3).max()
        print("  out %d x %d: iterations 3 - 2 %.3g px, 6 - 3 %.3g px, float32 %.3g px" %
              (out_size[1], out_size[0], np.abs(m3 - m2).max(), np.abs(m6 - m3).max(), spread))
        assert np.abs(m3 - m2).max() < 0.005 and np.abs(m6 - m3).max() < 1e-5
        assert 0 < spread <= MAP_SPREAD


def test_reference_renders_the_truth_at_the_smoothed_path():
    s, maps, truth = rr.scene(), sr.reference_maps(), sr.truth()
    for k in range(rr.N_FRAMES):
        ok = rr.inside(maps[k])
        img, n_out = rr.sample(s["frames"][k], maps[k])
        err = rr.grey_error(img, truth[k], ok)
        raw = rr.grey_error(s["frames"][k], truth[k], ok)
        print("frame %d: stabilised %.4f raw %.1f outside %.4f" % (rr.F0 + k, err, raw, n_out / ok.size))
        assert abs(err - sr.REFERENCE_ERROR[k]) <= 5e-4 and abs(raw - sr.RAW_ERROR[k]) <= 0.05, (k, err, raw)
        assert n_out == (~ok).sum() and abs(n_out / ok.size - sr.OUTSIDE_SHARE[k]) <= 5e-4
        assert err <= rr.RATIO * raw


@pytest.mark.parametrize("sigma", [0.1, 0.2])
def test_border_counts_fall_with_the_zoom_and_clear_borders_mean_clear_frames(sigma):
    from rssync_amd import synth
    s = rr.scene()
    g, lens, times = s["gyro"], s["lens"], s["times"]
    counts, _ = sr.coverage64(g, lens, rr.ROWS, rr.COLS, times, synth.D_TRUE, sr.ZOOMS, sigma=sigma)
    print("sigma %.1f:" % sigma, counts.tolist())
    assert (np.diff(counts, axis=1) <= 0).all()
    for k in range(rr.N_FRAMES):
        assert sr.first_clear(sr.ZOOMS, counts[k:k + 1]) == pytest.approx(sr.FIRST_CLEAR_ZOOM[sigma][k], abs=1e-12)
    assert counts[counts > 0].min() >= 127      # no rounding of a few 1e-4 px moves the chosen zoom
    assert sr.first_clear(sr.ZOOMS, counts) == pytest.approx(max(sr.FIRST_CLEAR_ZOOM[sigma]), abs=1e-12)
    # the whole frame at each frame's first clear zoom and one grid step below it: clear exactly where the border is
    for k in range(rr.N_FRAMES):
        z = int(np.argmax(counts[k] == 0))
        for zi in (z - 1, z):
            m = sr.map64(g, lens, rr.ROWS, rr.COLS, times[k], synth.D_TRUE, sigma=sigma, zoom=sr.ZOOMS[zi])
            full = int((~rr.inside(m)).sum())
            assert (full == 0) == (counts[k, zi] == 0), (k, zi, full, counts[k, zi])
            assert full >= counts[k, zi]


def test_border_enumeration_and_fixed_camera():
    b = sr.border(5, 7)
    assert b.shape == (2 * (5 + 7) - 4, 2) and len({tuple(p) for p in b}) == len(b)
    assert all(p[0] in (0, 6) or p[1] in (0, 4) for p in b)
    q = np.array([0.5, 0.5, -0.5, 0.5])
    np.testing.assert_array_equal(sr.fixed(q).orientation(np.zeros(3)), np.broadcast_to(q, (3, 4)))


def test_sampler_for_a_map_of_another_size_is_the_rectifiers():
    s, maps = rr.scene(), sr.reference_maps()
    want, want_n = rr.sample(s["frames"][0], maps[0], fill=9)
    got, got_n = sr.sample(s["frames"][0], maps[0], fill=9)
    np.testing.assert_array_equal(got, want)
    assert got_n == want_n > 0
    small, n = sr.sample(s["frames"][0], maps[0][::2, ::2], fill=9)
    np.testing.assert_array_equal(small, want[::2, ::2])
    assert n == int((~rr.inside(maps[0]))[::2, ::2].sum())


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


def test_library_exports_the_stabiliser_and_holds_its_kernels(built, tmp_path):
    import rssync_amd
    from rssync_amd import stabilize
    lib = rssync_amd.library_path()
    text = open(os.path.join(ROOT, "include", "rssync_stabilize.h")).read()
    declared = set(re.findall(r"\b(rssync_stabilize_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == {"rssync_stabilize_path", "rssync_stabilize_map", "rssync_stabilize_frames", "rssync_stabilize_coverage"}
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert not (declared - exported), sorted(declared - exported)
    assert declared <= set(stabilize.SIGNATURES)
    stabilize.library()                 # binds every signature: a missing symbol raises
    for name in ("stabilize_path", "stabilize_map", "stabilize_frames", "stabilize_coverage", "stabilize_zoom"):
        assert callable(getattr(rssync_amd.SyncProblem, name)) and callable(getattr(stabilize, name))
    # the code object: every stabiliser kernel is there and has no private segment
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    private = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "stabilize" in name:
            private[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\S+)", block).group(1))
    for want in ("stabilize_path_kernel", "stabilize_rows_kernel", "stabilize_kernelILi0ELb0", "stabilize_kernelILi0ELb1",
                 "stabilize_kernelILi1ELb0", "stabilize_kernelILi1ELb1", "stabilize_coverage_kernel"):
        assert [n for n in private if want in n], (want, sorted(private))
    assert not any(private.values()), private
