"""The path limiter without a GPU: its numpy restatement (tests/limit_reference.py) on the two shared cases, the lower
envelope's properties, csrc/limit_math.hpp compiled for the CPU against the restatement, the public header as C99, what
the built library exports and holds, and the errors that are raised before a device is asked for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import limit_reference as lr
import stabilize_reference as sr
import zoom_reference as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
CHECK = os.path.join(ROOT, "tests", "cpu_device", "limit_math_check.cpp")


@pytest.fixture(scope="module", params=sorted(lr.CASES))
def case(request):
    name = request.param
    return name, lr.CASES[name], lr.frames(name)


def test_reference_bisection_gives_the_recorded_strengths_in_all_three_readings(case):
    name, c, frames = case
    tol = sr.device_tolerance(c["camera"])
    for mode in (lr.PLAIN, lr.LIBERAL, lr.CONSERVATIVE):
        strengths, status = lr.fit64(frames, mode=mode, tol=tol)
        print(name, c["zoom"], mode, strengths.tolist())
        np.testing.assert_array_equal(strengths, np.array(lr.FITTED[name]))
        assert not status.any()
    # every value is the bisection's lo after ten steps: a multiple of 2^-10, exactly
    a = np.array(lr.FITTED[name])
    assert (a * 1024 == np.rint(a * 1024)).all()
    # what makes the case worth recording: some frames follow the goal all the way, several only part of it
    assert (a == 1).sum() >= 1 and ((a > 0) & (a < 1)).sum() >= 3


def test_reference_at_the_zoom_the_case_was_meant_for():
    """case A at 1.06: the plain and the liberal reading give the strengths the case was proposed with; the conservative
    one differs in frame 1 by one step, which is why the case's zoom is 1.059 (tests/limit_reference.py)"""
    frames = lr.frames("A", zoom=1.06)
    tol = sr.device_tolerance(sr.LENS)
    plain, _ = lr.fit64(frames)
    liberal, _ = lr.fit64(frames, mode=lr.LIBERAL, tol=tol)
    conservative, _ = lr.fit64(frames, mode=lr.CONSERVATIVE, tol=tol)
    np.testing.assert_array_equal(plain, np.array(lr.AT_106))
    np.testing.assert_array_equal(liberal, plain)
    assert (conservative <= plain).all() and (plain - conservative).tolist() == [0, 1 / 1024, 0, 0, 0, 0, 0, 0, 0]


def test_reference_frames_that_show_a_border_without_smoothing():
    """case A at zoom 1.0: the lens's camera at the frame's own size sees past the frame in every frame"""
    strengths, status = lr.fit64(lr.frames("A", zoom=lr.NOT_CLEAR_ZOOM["A"]))
    assert (strengths == 0).all() and (status == lr.NOT_CLEAR).all()


def test_clear_is_monotone_in_the_strength_on_the_recorded_frames(case):
    """what lets a smoothed strength, which is never above the fitted one, stay clear: observed, not proven"""
    name, c, frames = case
    grid = np.linspace(0.0, 1.0, 17)
    for f in (1, 3):
        clear = np.array([frames[f].clear(a) for a in grid])
        assert clear.any() and not clear.all()
        assert (np.diff(clear.astype(int)) <= 0).all(), (name, f, clear.tolist())


def test_bisect_follows_the_procedure_not_the_edge():
    assert lr.bisect(lambda a: a <= 0.3, 1) == (0.0, 0)
    assert lr.bisect(lambda a: a <= 0.3, 2) == (0.25, 0)
    assert lr.bisect(lambda a: a <= 1.5, 5) == (1.0, 0)
    assert lr.bisect(lambda a: a <= -0.5, 5) == (0.0, 1)
    # not monotone: clear up to 0.2 and on [0.6, 0.7): the first mid, 0.5, is not clear, so the search goes down
    assert lr.bisect(lambda a: a <= 0.2 or 0.6 <= a < 0.7, 3) == (0.125, 0)


def test_envelope_never_exceeds_and_a_window_of_zero_copies():
    rng = np.random.default_rng(3)
    for name in sorted(lr.FITTED):
        a = np.array(lr.FITTED[name])
        for window in (0.02, 1 / 30, 0.1, 0.5, 10.0):
            out = lr.smooth(lr.TIMES, a, window)
            assert (out <= a).all() and (out >= a.min()).all()
        np.testing.assert_array_equal(lr.smooth(lr.TIMES, a, 0.0), a)
        assert (lr.smooth(lr.TIMES, a, 0.02) == a).all()       # a window shorter than the frame spacing holds the frame alone
    t = np.sort(rng.random(200) * 6)
    t[50:53] = t[50]                                            # repeated times
    a = rng.random(200)
    for window in (0.05, 0.3, 2.0):
        out = lr.smooth(t, a, window)
        assert (out <= a).all() and (out >= a.min()).all()


def test_envelope_is_the_zoom_envelope_mirrored():
    """min and max exchanged: the envelope of 2 - a is 2 minus the zoom envelope of a, up to the rounding of the mean"""
    a = np.array(lr.FITTED["A"])
    np.testing.assert_allclose(lr.smooth(lr.TIMES, a, 0.1), 2 - zr.smooth(lr.TIMES, 2 - a, 0.1), rtol=1e-14)


def _run_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, CHECK], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def header_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("limit_check")
    plain = _run_check(d, "plain", [])
    # host code in a stand-alone program: the sanitizers' runtimes are linked in, nothing is preloaded
    checked = _run_check(d, "sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    return plain, checked


def _rows(text, tag):
    return [line.split()[1:] for line in text.splitlines() if line.startswith(tag + " ")]


def test_header_bisection_is_the_restatements(header_output):
    plain, checked = header_output
    assert plain == checked, "the sanitized build printed something else"
    rows = _rows(plain, "b")
    assert len(rows) == 13 * 11 + 2
    assert {int(r[0]) for r in rows} == set(range(1, 13)) | {40}
    seen = set()
    for steps, c, a, status in rows:
        c, steps = float.fromhex(c), int(steps)
        if c < -0.5:
            want = lr.bisect(lambda v: v <= 0.2 or 0.6 <= v < 0.7, steps)
        else:
            want = lr.bisect(lambda v: v <= c, steps)
            seen.add("below" if c < 0 else ("above" if c >= 1 else "in"))
        assert (float(want[0]).hex(), want[1]) == (float.fromhex(a).hex(), int(status)), (steps, c)
    assert seen == {"below", "above", "in"}
    # all three branches: strength 1, NOT_CLEAR, and a bisected value
    got = {(float.fromhex(r[2]), int(r[3])) for r in rows}
    assert (1.0, 0) in got and (0.0, 1) in got and any(0 < a < 1 and st == 0 for a, st in got)


PAIRS = (((0.9238795325112867, 0.1, -0.2, 0.31), (0.88, 0.17, -0.29, 0.33)),
         ((0.9238795325112867, 0.1, -0.2, 0.31), (-0.88, -0.17, 0.29, -0.33)),
         ((0.3, -0.7, 0.2, 0.61), (0.66, -1.3, 0.5, 1.1)))


def test_header_blend_and_normalisation_are_the_restatements_bit_for_bit(header_output):
    plain, _ = header_output
    blends, units = _rows(plain, "m"), _rows(plain, "u")
    assert len(blends) == len(units) == 18
    for m, u in zip(blends, units):
        p, a = int(m[0]), float.fromhex(m[1])
        r, g = np.array(PAIRS[p][0]), np.array(PAIRS[p][1])
        got = np.array([float.fromhex(v) for v in m[2:]])
        want = lr.blend(r, g, a)
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
        if a == 0:
            np.testing.assert_array_equal(got.view(np.uint64), r.view(np.uint64))
        if a == 1:
            np.testing.assert_array_equal(got.view(np.uint64), g.view(np.uint64))
        got_u = np.array([float.fromhex(v) for v in u[2:6]])
        np.testing.assert_array_equal(got_u.view(np.uint64), lr.unit(want).view(np.uint64))
        assert float.fromhex(u[6]) == np.sqrt(((want[0] * want[0] + want[1] * want[1]) + want[2] * want[2]) + want[3] * want[3])
    # the sign rule: a goal given with the opposite sign gives the same candidate between the ends
    for m0, m1 in zip(blends[:6], blends[6:12]):
        a = float.fromhex(m0[1])
        if 0 < a < 1:
            assert m0[2:] == m1[2:], (a, m0, m1)
        elif a == 1:
            assert [float.fromhex(v) for v in m0[2:]] == [-float.fromhex(v) for v in m1[2:]]


def test_header_envelope_against_the_restatement(header_output):
    """two exp implementations may differ by an ulp per weight and nothing else differs: 1e-12 relative"""
    plain, _ = header_output
    got = np.array([float.fromhex(r[0]) for r in _rows(plain, "w")])
    copy = np.array([float.fromhex(r[0]) for r in _rows(plain, "c")])
    flat = np.array([float.fromhex(r[0]) for r in _rows(plain, "k")])
    a = np.array(lr.FITTED["A"])
    want = lr.smooth(lr.TIMES, a, lr.WINDOW)
    worst = float(np.abs(got / want - 1).max())
    print("envelope against numpy: %.3g relative" % worst)
    assert got.shape == want.shape and worst <= 1e-12
    assert (got <= a).all() and (got < a).any() and (got >= a.min()).all()
    np.testing.assert_array_equal(copy, a)
    assert flat.shape == (9,) and (flat == 0.625).all()


def test_public_header_is_c99(tmp_path):
    src = tmp_path / "limit.c"
    src.write_text('#include "rssync_limit.h"\n'
                   'int main(void) { return (RSSYNC_LIMIT_CLEAR == 0 && RSSYNC_LIMIT_NOT_CLEAR == 1) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o",
                    str(tmp_path / "limit.o"), str(src)], check=True)


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


def test_library_exports_the_limiter_and_holds_its_kernel(built, tmp_path):
    import rssync_amd
    from rssync_amd import limit
    lib = rssync_amd.library_path()
    text = open(os.path.join(ROOT, "include", "rssync_limit.h")).read()
    declared = set(re.findall(r"\b(rssync_limit_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == {"rssync_limit_fit", "rssync_limit_smooth", "rssync_limit_targets"}
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {e for e in exported if e.startswith("rssync_limit_")} == declared
    assert declared <= set(limit.SIGNATURES)
    limit.library()                     # binds every signature: a missing symbol raises
    for name in ("fit_strength", "smooth_strengths", "limited_targets"):
        assert callable(getattr(rssync_amd.SyncProblem, name)) and callable(getattr(limit, name))
    # the code object: one kernel of the limiter, which needs neither scratch nor spills
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "limit_" in name:
            found[name] = {k: int(re.search(r"\.%s:\s+(\S+)" % k, block).group(1))
                           for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    print(found)
    assert len(found) == 1 and "limit_fit_kernel" in next(iter(found)), sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)


def test_errors_raised_before_a_device_is_asked_for(built):
    """what can be reached without a problem: the pointer, window and sigma checks in front of the problem's own, and the
    missing problem itself.  The rest: tests/test_gpu_limit.py."""
    from rssync_amd import limit, stabilize
    lib = limit.library()
    lib.rssync_set_panic_mode(1)
    PD = C.POINTER(C.c_double)
    t = np.array(lr.TIMES)
    a = np.array(lr.FITTED["A"])
    out = np.zeros(9)
    q = np.zeros((9, 4))
    L = np.ones(9)
    prm = stabilize.params(sigma=lr.SIGMA)
    st = np.zeros(9, np.uint32)

    def pd(v):
        return None if v is None else v.ctypes.data_as(PD)

    def err():
        return lib.rssync_last_error().decode()

    def fit(times=t, strengths=out):
        return lib.rssync_limit_fit(None, 380, 676, L.ctypes.data, 380, 676, pd(times), 9, 0.0, None, C.byref(prm), None, 10, pd(strengths),
                                    st.ctypes.data_as(C.POINTER(C.c_uint32)))

    for match, kw in (("no frame times", dict(times=None)), ("null output", dict(strengths=None)), ("no problem", dict())):
        assert fit(**kw) != 0, kw
        assert match in err(), (match, err())
    for match, args in (("no problem", (pd(t), pd(a), 9, 0.1, pd(out))), ("no problem", (pd(t), pd(a), 9, -1.0, pd(out)))):
        assert lib.rssync_limit_smooth(None, *args) != 0
        assert match in err(), (match, err())

    def targets(times=t, strengths=a, o=q, sigma=0.2):
        return lib.rssync_limit_targets(None, pd(times), 9, 0.01, 0.0, None, sigma, pd(strengths), pd(o))

    for match, kw in (("no frame times", dict(times=None)), ("no strengths", dict(strengths=None)), ("null output", dict(o=None)),
                      ("sigma", dict(sigma=-1.0)), ("sigma", dict(sigma=float("nan"))), ("no problem", dict())):
        assert targets(**kw) != 0, kw
        assert match in err(), (match, err())
    assert (out == 0).all() and (q == 0).all()
