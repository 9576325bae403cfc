"""The tracker (include/rssync_track.h) without a GPU: what the product library exports, what the code object holds for
its two kernels, and the numpy reference tracker (tests/track_reference.py) the GPU tests compare the kernels with --
checked here against shifts it must recover and against the synthetic video's ground truth (rs-sync_amd/synth_video.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import track_reference as tr
from track_scenes import shifted_pair as _shifted_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rs-sync_amd", "librssync_core.so")
LLVM = "/opt/rocm/lib/llvm/bin"

# Measured with this file's render (6 frames, half-resolution lens, step 100: 5 x 91 points): error of the reference
# tracker against the renderer's ground truth at the points of status 0, median 0.068 px, largest 1.25 px.  The bounds
# leave room for a different libm, not for a different tracker.
RENDER_MEDIAN_PX = 0.075
RENDER_MAX_PX = 1.4


def _declared():
    with open(os.path.join(ROOT, "include", "rssync_track.h")) as f:
        return re.findall(r"^int (rssync_track_\w+)\(", f.read(), flags=re.M)


def test_product_exports_every_declared_entry_point(built):
    names = _declared()
    assert sorted(names) == ["rssync_track_frames", "rssync_track_points"]
    lib = ctypes.CDLL(LIB)
    for name in names:
        assert hasattr(lib, name), name
    from rssync_amd import track
    assert set(names) <= set(track.SIGNATURES)
    track.library()                                     # binds without a device


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


def test_code_object_holds_the_tracker_kernels(built, tmp_path):
    """pyr_down_kernel (both input types) and lk_kernel are in the shipped code object: no scratch, no spills, no private
    segment, no matrix instructions; eight waves per SIMD for the pyramid, four for LK (104 VGPRs: 21 fp32 template and
    gradient values per lane plus the level loop's state)"""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, LIB, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        def get(key):
            return re.search(r"\.%s:\s+(\S+)" % key, block).group(1)
        name = get("name")
        if "pyr_down_kernel" in name or "lk_kernel" in name:
            found[name] = {k: int(get(k)) for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count",
                                                      "sgpr_spill_count", "group_segment_fixed_size")}
    pyr = {n: k for n, k in found.items() if "pyr_down_kernel" in n}
    lk = {n: k for n, k in found.items() if "lk_kernel" in n}
    assert len(pyr) == 2 and len(lk) == 1, sorted(found)
    for n, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
    assert all(512 // k["vgpr_count"] >= 8 and k["group_segment_fixed_size"] <= 8 * 1024 for k in pyr.values()), pyr
    assert all(512 // k["vgpr_count"] >= 4 for k in lk.values()), lk
    dis = subprocess.run([_tool("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    funcs = re.split(r"^[0-9a-f]+ <(\S+)>:$", dis, flags=re.M)
    bodies = {n: b for n, b in zip(funcs[1::2], funcs[2::2]) if n in found}
    assert set(bodies) == set(found)
    for n, b in bodies.items():
        assert not re.search(r"\bscratch_(load|store)", b) and "v_mfma" not in b, n


def _driver_grid(width, height, step):
    out = []
    for i in range(step, width, step):       # core_testcode.cpp:124-132, outer loop over x
        for j in range(step, height, step):
            out.append((i, j))
    return out


@pytest.mark.parametrize("w,h,step", [(2704, 2028, 200), (2704, 1520, 200), (1352, 760, 100), (201, 201, 200),
                                      (200, 600, 200), (37, 29, 5), (17, 16, 16), (50, 50, 60), (1, 1, 1)])
def test_grid_is_the_drivers_loop(w, h, step):
    from rssync_amd import track
    want = np.array(_driver_grid(w, h, step), np.float64).reshape(-1, 2)
    np.testing.assert_array_equal(track.grid(w, h, step), want)
    np.testing.assert_array_equal(tr.grid(w, h, step), want)
    assert len(want) == max(0, (w - 1) // step) * max(0, (h - 1) // step)
    if (w, h, step) == (2704, 2028, 200):
        assert len(want) == 130                                 # the bench's reference driver workload


def test_reference_recovers_integer_shifts():
    for sx, sy in ((7, -4), (-23, 11), (0, 0)):
        pa, pb, st, _ = tr.track(_shifted_pair(sx, sy, 16, 64), step=70)
        assert (st == 0).all(), st
        assert np.abs(pb[0] - pa - (sx, sy)).max() <= 1e-3, (sx, sy, np.abs(pb[0] - pa - (sx, sy)).max())


def test_reference_recovers_subpixel_shifts():
    """Bilinear LK over an unweighted window is biased at a fractional shift f: to first order the bias is
    f (1 - f) / 2 * [B'^2] over the window's edges / sum(B'^2) -- a window-edge term, ~0.01 px on average for a 21 x 21
    window, larger at single points.  Measured on this texture (12 .. 60 px): median 0.009 .. 0.012 px, largest
    0.022 .. 0.037 px over the 20 points of each shift."""
    for sx, sy in ((0.25, 0.5), (-3.7, 2.3), (12.4, -0.15), (0.5, 0.0)):
        pa, pb, st, _ = tr.track(_shifted_pair(sx, sy, 12, 60), step=70)
        assert (st == 0).all(), st
        err = np.linalg.norm(pb[0] - pa - (sx, sy), axis=-1)
        assert np.median(err) <= 0.0125 and err.max() <= 0.04, (sx, sy, np.median(err), err.max())


def test_pyramid_sizes_and_level_one_is_exact():
    rng = np.random.default_rng(1)
    f = rng.integers(0, 256, size=(29, 37), dtype=np.uint8)
    pyr = tr.pyramid(f, 4)
    assert [p.shape for p in pyr] == [(29, 37), (15, 19), (8, 10), (4, 5)]
    # level 1 in float64 with an explicit reflect-101 pad: the same numbers (integer sums below 2^24)
    k = np.array([1, 4, 6, 4, 1], np.float64)
    pad = np.pad(f.astype(np.float64), 2, mode="reflect")
    full = np.apply_along_axis(lambda r: np.convolve(r, k, "valid"), 1, pad)
    full = np.apply_along_axis(lambda c: np.convolve(c, k, "valid"), 0, full) / 256.0
    np.testing.assert_array_equal(pyr[1], full[::2, ::2].astype(np.float32))


def test_reference_on_the_rendered_video():
    """against the ground truth of the renderer (a's ray meets the box, re-projected with the row-time iteration)"""
    from rssync_amd import synth, synth_video as sv
    g = synth.make_gyro(1.0, 1.0 + 10 / synth.FPS, seed=77)
    lens = sv.half_lens()
    frames, _ = sv.render(g, 30, 36, lens=lens, rows=760, cols=1352, seed=77)
    pa, pb, st, res = tr.track(frames, step=100)
    assert pa.shape == (91, 2)
    truth = sv.true_points(g, 30, 36, pa, lens=lens, rows=760, seed=77)
    err = np.linalg.norm(pb - truth, axis=-1)
    ok = st == 0
    assert ok.mean() >= 0.95, np.bincount(st.ravel())
    assert np.median(err[ok]) < RENDER_MEDIAN_PX and err[ok].max() < RENDER_MAX_PX, (np.median(err[ok]), err[ok].max())
    assert np.isfinite(res).all()


def test_diagnostics_leave_the_results_unchanged():
    pair = _shifted_pair(3.3, -1.6, 12, 60, w=200, h=160)
    pyrs = [tr.pyramid(f, 3) for f in pair]
    pts = tr.grid(200, 160, 30)
    kw = dict(window=9, max_iters=5, epsilon=0.05, min_eig=2.0)
    plain = tr.track_pair(pyrs[0], pyrs[1], pts, **kw)
    flow, st, res, m = tr.track_pair(pyrs[0], pyrs[1], pts, diag=True, **kw)
    for a, b in zip(plain, (flow, st, res)):
        np.testing.assert_array_equal(a, b)
    assert set(m) == {"eig", "det", "conv", "border", "left_level"}
    assert all(v.shape == (len(pts),) for v in m.values())


def test_a_point_on_the_min_eig_bound_is_near_a_decision():
    """min_eig set to a point's own level-0 eigenvalue: that point's test is decided by rounding (fp64 passes it, the
    kernel's fp32 may not), so it is excused; min_eig a hair above makes it ill-conditioned and is excused as well"""
    pair = _shifted_pair(0.3, 0.2, 12, 60, w=120, h=120)
    pyrs = [tr.pyramid(f, 2) for f in pair]
    pts = np.array([[60.0, 60.0], [40.0, 70.0]])
    me = tr.min_eigenvalue(pair[0], pts)
    assert me[0] > 1.0                                       # textured: far from the default bound
    for bound, want in ((me[0], tr.STATUS_OK), (me[0] * (1 + 1e-9), tr.STATUS_ILL)):
        _, st, _, m = tr.track_pair(pyrs[0], pyrs[1], pts[:1], min_eig=bound, diag=True)
        assert st[0] == want
        assert m["eig"][0] < 1e-8 and tr.near_decision(m, 0.01)[0]


def test_a_plain_interior_point_is_not_near_a_decision():
    pair = _shifted_pair(0.3, 0.2, 12, 60, w=120, h=120)
    pyrs = [tr.pyramid(f, 2) for f in pair]
    flow, st, _, m = tr.track_pair(pyrs[0], pyrs[1], np.array([[60.0, 60.0]]), diag=True)
    assert st[0] == tr.STATUS_OK and not tr.near_decision(m, 0.01)[0], m
    assert m["border"][0] > 20 and m["eig"][0] > 1e-2 and m["det"][0] > 1e-2 and m["left_level"][0] == -1
    assert np.isfinite(m["conv"][0])                         # it took convergence tests: it has a margin


def test_border_margins_count_moved_positions_only():
    """identical frames: the flow stays exactly 0, so a point on column width-1 sits exactly on the border line in fp32
    as in fp64 -- no split is possible and nothing is excused.  Moved by a sub-pixel shift, the same point's border tests
    have a margin: its distance to the line."""
    pair = _shifted_pair(-0.3, 0.0, 12, 60, w=64, h=48)
    pyr = tr.pyramid(pair[0], 1)
    pts = np.array([[63.0, 20.0], [30.0, 20.0]])
    flow, st, _, m = tr.track_pair(pyr, pyr, pts, diag=True)
    assert (st == tr.STATUS_OK).all() and (flow == 0).all()
    assert np.isinf(m["border"]).all() and not tr.near_decision(m, 0.01).any()
    flow, st, _, m = tr.track_pair(pyr, tr.pyramid(pair[1], 1), pts, diag=True)
    assert st[0] == tr.STATUS_OK and 0 < m["border"][0] <= abs(flow[0, 0]) + 1e-12, (flow[0], m["border"][0])
    assert 19 < m["border"][1] < 21 and not tr.near_decision(m, 0.01)[1]


def test_a_point_carried_out_at_a_coarse_level_records_that_level():
    """a 40 px shift at level 3 of a 160 px wide frame: the points near the right edge leave there"""
    pair = _shifted_pair(40.0, 0.0, 16, 64, w=160, h=96)
    pyrs = [tr.pyramid(f, 4) for f in pair]
    pts = tr.grid(160, 96, 16)
    _, st, _, m = tr.track_pair(pyrs[0], pyrs[1], pts, diag=True)
    coarse = m["left_level"] > 0
    assert coarse.any() and (st[coarse] == tr.STATUS_LEFT).all()
    assert (m["left_level"][st != tr.STATUS_LEFT] == -1).all()
