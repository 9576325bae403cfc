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


def _texture(x, y, lo, hi, seed=5):
    """band-limited pattern evaluated exactly at any position: 16 sinusoids, wavelengths lo .. hi px, every direction"""
    rng = np.random.default_rng(seed)
    v = np.zeros(np.broadcast(x, y).shape)
    for _ in range(16):
        lam, th, ph = rng.uniform(lo, hi), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        v += np.sin(2 * np.pi / lam * (np.cos(th) * x + np.sin(th) * y) + ph)
    return np.clip(np.rint(128 + 30 * v), 0, 255).astype(np.uint8)


def _shifted_pair(sx, sy, lo, hi, w=420, h=340):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([_texture(xs, ys, lo, hi), _texture(xs - sx, ys - sy, lo, hi)])   # content moves by (+sx, +sy)


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
