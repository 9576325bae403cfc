"""The dynamic zoom without a GPU: its numpy restatement (tests/zoom_reference.py) on the two shared cases, the envelope's
properties, csrc/zoom_math.hpp compiled for the CPU against the restatement, the public header as C99, and what the built
library exports and holds."""
import os
import re
import subprocess

import numpy as np
import pytest

import stabilize_reference as sr
import zoom_reference as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
CHECK = os.path.join(ROOT, "tests", "cpu_device", "zoom_math_check.cpp")


@pytest.fixture(scope="module", params=sorted(zr.CASES))
def case(request):
    name = request.param
    return name, zr.CASES[name], zr.borders(name)


def test_reference_bisection_gives_the_recorded_zooms_in_all_three_readings(case):
    name, c, frames = case
    tol = sr.device_tolerance(c["camera"])
    for mode in (zr.PLAIN, zr.LIBERAL, zr.CONSERVATIVE):
        zooms, status = zr.fit64(frames, c["lo"], c["hi"], mode=mode, tol=tol)
        print(name, mode, zooms.tolist())
        np.testing.assert_array_equal(zooms, np.array(zr.FITTED[name]))
        assert not status.any()
    # every value is the bisection's hi after ten steps: lo plus a multiple of (hi - lo) / 1024, exactly
    steps = (np.array(zr.FITTED[name]) - c["lo"]) / ((c["hi"] - c["lo"]) / 1024)
    assert (steps == np.rint(steps)).all() and (steps > 0).all() and (steps < 1024).all()


def test_clear_is_monotone_over_the_range(case):
    """what lets a smoothed zoom, which is never below the fitted one, stay clear"""
    name, c, frames = case
    grid = np.linspace(c["lo"], c["hi"], 41)
    for f in (0, 4, 8):      # k = 31, 35, 39
        clear = np.array([frames[f].clear(z) for z in grid])
        assert clear.any() and not clear.all()
        assert (np.diff(clear.astype(int)) >= 0).all(), (name, f, clear.tolist())
        first = grid[int(np.argmax(clear))]
        assert first - (c["hi"] - c["lo"]) / 40 < zr.FITTED[name][f] <= first


def test_statuses_of_the_reference():
    frames = zr.borders("A")
    zooms, status = zr.fit64(frames, 1.0, 1.02)
    assert (zooms == 1.02).all() and (status == zr.NOT_CLEAR).all()
    zooms, status = zr.fit64(frames, 1.2, 1.5)
    assert (zooms == 1.2).all() and (status == zr.CLEAR).all()
    zooms, status = zr.fit64(frames, 1.0, 1.06)
    assert status.tolist() == [0, 1, 1, 1, 0, 0, 0, 1, 1]
    assert (zooms[status == 1] == 1.06).all() and (zooms[status == 0] < 1.06).all()


def test_bisect_follows_the_procedure_not_the_edge():
    assert zr.bisect(lambda z: z >= 1.3, 1.0, 1.5, 1) == (1.5, 0)
    assert zr.bisect(lambda z: z >= 1.3, 1.0, 1.5, 2) == (1.375, 0)
    assert zr.bisect(lambda z: z >= 1.6, 1.0, 1.5, 5) == (1.5, 1)
    assert zr.bisect(lambda z: z >= 0.2, 1.0, 1.5, 5) == (1.0, 0)
    # not monotone: clear on [1.1, 1.2) and from 1.4: the first mid, 1.25, is not clear, so the search goes up
    assert zr.bisect(lambda z: z >= 1.4 or 1.1 <= z < 1.2, 1.0, 1.5, 3) == (1.4375, 0)


def test_envelope_never_undercuts_and_a_window_of_zero_copies():
    rng = np.random.default_rng(3)
    for name in sorted(zr.FITTED):
        z = np.array(zr.FITTED[name])
        for window in (0.02, 1 / 30, 0.1, 0.5, 10.0):
            out = zr.smooth(zr.TIMES, z, window)
            assert (out >= z).all() and (out <= z.max()).all()
        np.testing.assert_array_equal(zr.smooth(zr.TIMES, z, 0.0), z)
        assert (zr.smooth(zr.TIMES, z, 0.02) == z).all()       # a window shorter than the frame spacing holds the frame alone
    t = np.sort(rng.random(200) * 6)
    t[50:53] = t[50]                                            # repeated times
    z = 1 + rng.random(200)
    for window in (0.05, 0.3, 2.0):
        out = zr.smooth(t, z, window)
        assert (out >= z).all() and (out <= z.max()).all()


def test_envelope_of_a_single_spike():
    t = np.arange(61) / 30
    for at in (0, 17, 60):
        for h, window in ((1.5, 0.25), (1.01, 0.5), (3.0, 1 / 30)):
            z = np.ones(61)
            z[at] = h
            out = zr.smooth(t, z, window)
            assert (out <= h).all() and out[at] == h and (out >= 1).all()
            assert (np.diff(out[at:]) <= 0).all() and (np.diff(out[:at + 1]) >= 0).all()
            assert (out[np.abs(t - t[at]) > 2 * window + 1e-9] == 1).all()      # (the spike's reach: two windows)


def _run_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, CHECK], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def header_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("zoom_check")
    plain = _run_check(d, "plain", [])
    # host code in a stand-alone program: the sanitizers' runtimes are linked in, nothing is preloaded
    checked = _run_check(d, "sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    return plain, checked


def test_header_bisection_is_the_restatements(header_output):
    plain, checked = header_output
    assert plain == checked, "the sanitized build printed something else"
    rows = [line.split()[1:] for line in plain.splitlines() if line.startswith("b ")]
    assert len(rows) == 3 * 4 * 12 + 2
    seen = set()
    for lo, hi, steps, c, zoom, status in rows:
        lo, hi, c, steps = float.fromhex(lo), float.fromhex(hi), float.fromhex(c), int(steps)
        if c < 0:
            want = zr.bisect(lambda z: z >= 1.4 or 1.1 <= z < 1.2, lo, hi, steps)
        else:
            want = zr.bisect(lambda z: z >= c, lo, hi, steps)
        assert (float(want[0]).hex(), want[1]) == (float.fromhex(zoom).hex(), int(status)), (lo, hi, steps, c)
        seen.add("below" if c < lo else ("above" if c > hi else "in"))
    assert seen == {"below", "above", "in"}
    assert {int(r[5]) for r in rows} == {0, 1}


def test_header_envelope_against_the_restatement(header_output):
    """two exp implementations may differ by an ulp per weight and nothing else differs: 1e-12 relative"""
    plain, _ = header_output
    got = np.array([float.fromhex(line.split()[1]) for line in plain.splitlines() if line.startswith("w ")])
    copy = np.array([float.fromhex(line.split()[1]) for line in plain.splitlines() if line.startswith("c ")])
    z = np.array(zr.FITTED["A"])
    want = zr.smooth(zr.TIMES, z, zr.WINDOW)
    worst = float(np.abs(got / want - 1).max())
    print("envelope against numpy: %.3g relative" % worst)
    assert got.shape == want.shape and worst <= 1e-12
    assert (got >= z).all() and (got > z).any()
    np.testing.assert_array_equal(copy, z)


def test_public_header_is_c99(tmp_path):
    src = tmp_path / "zoom.c"
    src.write_text('#include "rssync_zoom.h"\n'
                   'int main(void) { return (RSSYNC_ZOOM_CLEAR == 0 && RSSYNC_ZOOM_NOT_CLEAR == 1) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o",
                    str(tmp_path / "zoom.o"), str(src)], check=True)


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


ZOOM_KERNELS = ["zoom_fit_kernel"] + ["zoom_render_kernelILi%dELi%dE" % (c, f) for c in (0, 1) for f in (0, 1)]


def test_library_exports_the_dynamic_zoom_and_holds_its_kernels(built, tmp_path):
    import rssync_amd
    from rssync_amd import zoom
    lib = rssync_amd.library_path()
    text = open(os.path.join(ROOT, "include", "rssync_zoom.h")).read()
    declared = set(re.findall(r"\b(rssync_zoom_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == {"rssync_zoom_fit", "rssync_zoom_smooth", "rssync_zoom_stabilize"}
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {e for e in exported if e.startswith("rssync_zoom_")} == declared
    assert declared <= set(zoom.SIGNATURES)
    zoom.library()                      # binds every signature: a missing symbol raises
    for name in ("fit_zoom", "smooth_zooms", "dynamic_zoom", "stabilize_frames_zoomed", "stabilize_frames_zoomed_budget"):
        assert callable(getattr(rssync_amd.SyncProblem, name)) and callable(getattr(zoom, name))
    # the code object: every kernel of the dynamic zoom is there, once, and needs neither scratch nor spills
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "zoom" in name:
            found[name] = {k: int(re.search(r"\.%s:\s+(\S+)" % k, block).group(1))
                           for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    for want in ZOOM_KERNELS:
        hit = [n for n in found if want in n]
        assert len(hit) == 1, (want, sorted(found))
        print(want, found[hit[0]])
    assert len(found) == len(ZOOM_KERNELS), sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
