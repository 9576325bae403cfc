"""The feature tracker (include/rssync_features.h) without a GPU: what the product library exports and the Python layer
binds, what the code object holds for its kernels, the numpy detector (tests/feature_reference.py) the GPU tests compare
the kernels with, and the renderer's flat regions (rs-sync_amd/synth_video.py)."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import feature_cases as fc
import feature_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rs-sync_amd", "librssync_core.so")
HEADER = os.path.join(ROOT, "include", "rssync_features.h")
LLVM = "/opt/rocm/lib/llvm/bin"


def _declared():
    with open(HEADER) as f:
        return re.findall(r"^int (rssync_features_\w+)\(", f.read(), flags=re.M)


def test_product_exports_and_binds_every_declared_entry_point(built):
    names = _declared()
    assert sorted(names) == ["rssync_features_frames", "rssync_features_track"]
    lib = ctypes.CDLL(LIB)
    for name in names + ["rship_features_track", "rship_track_list"]:
        assert hasattr(lib, name), name
    from rssync_amd import features
    assert set(names) <= set(features.SIGNATURES)
    features.library()                                  # binds without a device
    assert ctypes.sizeof(features.FeatureParams) == 64      # 4 + 4 + 8 + 8 + 4 (+ 4 padding: lk holds doubles) + 32


def test_header_is_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "rssync_features.h"\nint main(void) { rssync_feature_params p = {0}; (void)p; '
                   'return RSSYNC_FEATURE_FB_MISMATCH - 4; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


def test_code_object_holds_the_feature_kernels(built, tmp_path):
    """corner_cell_kernel, corner_select_kernel and both lkfb_kernel instantiations: no scratch, no spills, no private
    segment, no matrix instructions; LK at four waves per SIMD like lk_kernel, the detector's static LDS (the row ring)
    small enough that the byte tile of a 128-px cell (140 x 140) still leaves several workgroups per CU"""
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
        if "corner_cell_kernel" in name or "corner_select_kernel" in name or "lkfb_kernel" in name:
            found[name] = {k: int(get(k)) for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count",
                                                      "sgpr_spill_count", "group_segment_fixed_size")}
    cell = [k for n, k in found.items() if "corner_cell_kernel" in n]
    sel = [k for n, k in found.items() if "corner_select_kernel" in n]
    lk = [k for n, k in found.items() if "lkfb_kernel" in n]
    assert len(cell) == 1 and len(sel) == 1 and len(lk) == 2, sorted(found)
    for n, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
    assert all(512 // k["vgpr_count"] >= 4 for k in lk), lk
    assert cell[0]["group_segment_fixed_size"] + 140 * 140 <= 160 * 1024 // 4, cell   # >= 4 workgroups per CU at cell 128
    dis = subprocess.run([_tool("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    funcs = re.split(r"^[0-9a-f]+ <(\S+)>:$", dis, flags=re.M)
    bodies = {n: b for n, b in zip(funcs[1::2], funcs[2::2]) if n in found}
    assert set(bodies) == set(found)
    for n, b in bodies.items():
        assert not re.search(r"\bscratch_(load|store)", b) and "v_mfma" not in b, n


def _checkerboard(h=192, w=256, side=64, lo=50, hi=200):
    """squares of `side` px shifted by side / 2: one inner corner per side x side cell, at the pixel boundary
    (side / 2 + side i - 0.5, side / 2 + side j - 0.5)"""
    y, x = np.mgrid[0:h, 0:w]
    return np.where(((x + side // 2) // side + (y + side // 2) // side) % 2 == 1, hi, lo).astype(np.uint8)


def test_checkerboard_corners_one_per_cell():
    """The response of an ideal corner at (c - 0.5, c - 0.5) is symmetric under the reflections about it, so it peaks at
    four mirror pixels of equal R, block / 2 - 0.5 px from the corner inside each quadrant.  The tie goes to the smallest
    raster index, the up-left one: (c - block / 2, c - block / 2), for c = 32 + 64 i."""
    img = _checkerboard()
    for block in (3, 5, 7, 9):
        got = fr.detect(img, cell=64, block=block)
        o = 32 - block // 2
        want = np.array([(64 * i + o, 64 * j + o) for i in range(4) for j in range(3)])   # cells x-major
        np.testing.assert_array_equal(got, want, err_msg="block %d" % block)
        R = fr.response(img, block)
        m = 2 * (block // 2) - 1                          # the mirror offset
        for x, y in want:
            assert R[y, x] == R[y, x + m] == R[y + m, x] == R[y + m, x + m] > 0


def test_no_features_on_flat_frames_and_ramps():
    ramp = np.tile(np.arange(256, dtype=np.uint8), (100, 1))
    for img in (np.full((90, 120), 77, np.uint8), ramp, ramp.T.copy(), np.zeros((40, 40), np.uint8)):
        R = fr.response(img, 5)
        assert R[R != fr.NO_RESPONSE].max() <= 0
        assert fr.detect(img).shape == (0, 2)


def test_local_maxima_ties_go_to_the_smaller_raster_index():
    NO = fr.NO_RESPONSE
    R = np.full((6, 7), NO, np.int64)
    R[1:5, 1:6] = 0
    R[2, 2] = R[2, 3] = R[3, 2] = R[3, 3] = 50            # a 2 x 2 plateau: only its first pixel is a local maximum
    lm = fr.local_maxima(R)
    assert lm[2, 2] and lm.sum() == 1 + 0, np.argwhere(lm)
    R[4, 5] = 50                                           # a lone peak of the same height elsewhere
    R[1, 5] = 10                                           # and a smaller one whose neighbour (2, 4) is 0
    lm = fr.local_maxima(R)
    assert lm[2, 2] and lm[4, 5] and lm[1, 5] and lm.sum() == 3
    # NO_RESPONSE neighbours are not neighbours: a peak at the edge of the valid region counts
    R2 = np.full((3, 3), NO, np.int64)
    R2[1, 1] = -5
    assert fr.local_maxima(R2)[1, 1]


def test_detect_threshold_and_cell_winner():
    """two corners of equal response in one cell: the one with the smaller raster index wins; a cell whose best local
    maximum is below T has no feature"""
    img = np.full((64, 96), 40, np.uint8)
    img[10:20, 10:20] = 200                                # four corners of a square in cell (0, 0)
    img[40:44, 70:74] = 90                                 # a faint square in cell (1, 0)
    R = fr.response(img, 5)
    lm = fr.local_maxima(R)
    got = fr.detect(img, cell=48, block=5, quality=0.01)
    cell0 = [(x, y) for y, x in np.argwhere(lm) if x < 48 and y < 48]
    best = max(cell0, key=lambda p: (R[p[1], p[0]], -(p[1] * 96 + p[0])))
    assert tuple(got[0]) == best
    T = fr.threshold(R, 0.01)
    faint = max(R[y, x] for y, x in np.argwhere(lm) if x >= 48)
    assert faint >= T and len(got) == 2                   # the faint square passes at quality 0.01 ...
    assert faint < fr.threshold(R, 0.5) and len(fr.detect(img, cell=48, block=5, quality=0.5)) == 1   # ... not at 0.5


# --- the inputs of tests/test_gpu_feature_ties.py (tests/feature_cases.py) are not vacuous: by the numpy restatement alone
# they hold the ties, slivers, non-positive cells and list lengths that the device tests are there for


@pytest.mark.parametrize("h,w,P,seed", fc.TIE_FRAMES)
def test_tie_frames_hold_ties_in_every_configuration(h, w, P, seed):
    """Every (frame, configuration) of the device's tie test has pixels that tie with a neighbour for the local maximum
    (plateau) and pixels that only the tie rule rejects (dropped_by_tie); every frame has, at each cell size, cells whose
    winner is decided by the raster index alone.  kaleidoscope(197, 331, 13, 197): 2524 plateau pixels, 1262 dropped and
    170 tied cells at (16, 3, 1e-3); 18 of 18 cells tied at (64, 9, 0.01); 6 of 6 at (128, 5, 0.5); 84 features at
    (16, 9, 1.0)."""
    img = fc.kaleidoscope(h, w, P, seed)
    tied = {16: 0, 64: 0, 128: 0}
    for cell, block, quality in fc.TIE_CONFIGS:
        s = fc.tie_stats(img, cell, block, quality)
        print((h, w, P, seed), (cell, block, quality), s)
        assert s["plateau"] > 0 and s["dropped_by_tie"] > 0, ((cell, block, quality), s)
        assert s["kept"] > 0
        tied[cell] += s["cells_with_tied_best"]
    assert all(n > 0 for n in tied.values()), tied


def test_tie_frames_reach_every_stage_of_the_cell_reduction():
    """Over the case list, tied bests of one cell meet in one thread (corner_beats in the row loop), in two lanes of one
    wave (the shuffle butterfly) and in two waves (the reduction through LDS); see feature_cases.tie_paths.  Every frame
    reaches the last two on its own."""
    total = dict(thread=0, wave=0, workgroup=0)
    for h, w, P, seed in fc.TIE_FRAMES:
        img = fc.kaleidoscope(h, w, P, seed)
        mine = dict(thread=0, wave=0, workgroup=0)
        for cfg in fc.TIE_CONFIGS:
            for k, v in fc.tie_paths(img, *cfg).items():
                mine[k] += v
        print((h, w, P, seed), mine)
        assert mine["wave"] > 0 and mine["workgroup"] > 0, ((h, w), mine)
        for k in total:
            total[k] += mine[k]
    assert all(v >= 2 for v in total.values()), total


def test_quality_one_keeps_only_ties_for_the_maximum():
    """quality = 1.0: T = R_max.  On the periodic frames more than one cell holds a pixel of that response, and nothing
    else is listed (84 features on the 197 x 331 frame at cell 16, block 9)"""
    for h, w, P, seed in fc.TIE_FRAMES:
        img = fc.kaleidoscope(h, w, P, seed)
        for cell, block, quality in fc.TIE_CONFIGS:
            if quality != 1.0 or (cell >= h and cell >= w):
                continue
            R = fr.response(img, block)
            pts = fc.detect(img, cell, block, 1.0)
            assert fr.threshold(R, 1.0) == R.max()
            assert len(pts) >= 2 and (R[pts[:, 1], pts[:, 0]] == R.max()).all(), ((h, w), cell, block, len(pts))


def test_full_range_frame_stays_inside_the_number_formats():
    """The 0/255 kaleidoscope: the tensor sums fit int32 (the assert in fr.response), R_max < 2^53 so that the fp64
    threshold is exact, and block 9 reaches above 2^48 (508899560473125; 98 features at quality 1.0, cell 16).  The
    smallest quality gives T = 1."""
    img = fc.range_frame()
    assert set(np.unique(img)) == {0, 255}
    for block in fc.RANGE_BLOCKS:
        R = fr.response(img, block)                          # (asserts the int32 bound itself)
        r_max = int(R.max())
        print("block %d: r_max %d = 2^%.2f" % (block, r_max, np.log2(r_max)))
        assert 2 ** 43 < r_max < 2 ** 53
        assert float(r_max) == r_max
        assert fr.threshold(R, 1e-18) == 1 and fr.threshold(R, 1.0) == r_max
        for cell in fc.RANGE_CELLS:
            n = [len(fc.detect(img, cell, block, q)) for q in fc.RANGE_QUALITIES]
            assert 2 <= n[0] <= n[1] <= n[2] <= n[3], (block, cell, n)
    assert int(fr.response(img, 9).max()) > 2 ** 48


@pytest.mark.parametrize("block", fc.SLIVER_BLOCKS)
@pytest.mark.parametrize("cell", fc.SLIVER_CELLS)
def test_sliver_cells_are_empty_up_to_b_and_hold_one_line_at_b_plus_one(cell, block):
    """A last column and row of cells e px wide: no valid pixel, so no feature, at e = 1 and e = b = block // 2 + 1; one
    valid column (row) at e = b + 1, on which the reference lists at least one feature ((19, 35) at cell 16, block 3: 1
    in the last column of cells, 2 in the last row; (22, 38) at block 9: 1 and 2)"""
    b = block // 2 + 1
    for h, w, what in fc.sliver_sizes(cell, block):
        img = fc.sliver_frame(h, w)
        R = fr.response(img, block)
        n = fc.cell_counts(fc.detect(img, cell, block, fc.SLIVER_QUALITY), h, w, cell)
        last_col, last_row = int(n[-1].sum()), int(n[:, -1].sum())
        print(cell, block, (h, w), what, "last column %d, last row %d of %d" % (last_col, last_row, n.sum()))
        valid_col = (R[:, w // cell * cell:] != fr.NO_RESPONSE).any(axis=0).sum() if w % cell else None
        valid_row = (R[h // cell * cell:] != fr.NO_RESPONSE).any(axis=1).sum() if h % cell else None
        if what == "e=%d" % (b + 1):
            assert valid_col == 1 and valid_row == 1
            assert last_col >= 1 and last_row >= 1
        else:
            if w % cell:
                assert valid_col == 0 and last_col == 0
            if h % cell:
                assert valid_row == 0 and last_row == 0
        assert n.sum() >= 2                                  # (the full cells are not empty)


def test_patch_frame_has_cells_without_a_positive_response():
    """The textured frame with a constant rectangle and a ramp: thousands of valid pixels with R = 0 (5220) and with
    R < 0, some cells without a feature (112 of 140 kept at either quality), none of them strictly inside the rectangle"""
    img = fc.patch_frame()
    R = fr.response(img, fc.PATCH_BLOCK)
    v = R != fr.NO_RESPONSE
    print("R = 0: %d, R < 0: %d" % ((R[v] == 0).sum(), (R[v] < 0).sum()))
    assert (R[v] == 0).sum() >= 1000 and (R[v] < 0).sum() >= 1000
    y0, y1, x0, x1 = fc.PATCH_FLAT
    m = fc.PATCH_BLOCK // 2 + 1
    assert (R[y0 + m:y1 - m, x0 + m:x1 - m] == 0).all()
    y0, y1, x0, x1 = fc.PATCH_RAMP
    assert (R[y0 + m:y1 - m, x0 + m:x1 - m] < 0).all()
    cells = (-(-img.shape[0] // fc.PATCH_CELL)) * (-(-img.shape[1] // fc.PATCH_CELL))
    for q in fc.PATCH_QUALITIES:
        n = len(fc.detect(img, fc.PATCH_CELL, fc.PATCH_BLOCK, q))
        assert cells // 2 < n < cells - 10, (q, n, cells)


def test_round_frames_keep_every_cell():
    """255, 256 and 272 cells, each with a feature: the select kernel's list crosses its 256-thread round in full"""
    want = []
    for h, w in fc.ROUND_FRAMES:
        n = len(fc.detect(fc.round_frame(h, w), fc.ROUND_CELL, fc.ROUND_BLOCK, fc.ROUND_QUALITY))
        assert n == (h // fc.ROUND_CELL) * (w // fc.ROUND_CELL), (h, w, n)
        want.append(n)
    assert want == [255, 256, 272]


def test_mixed_batch_has_an_empty_frame_between_full_ones():
    n = [len(fc.detect(f, *fc.MIXED_CONFIG)) for f in fc.mixed_frames()]
    assert n[1] == 0 and n[0] == n[2] > 100 and n[3] > 100, n


# sha256 of render(make_gyro(1.0, 1.0 + 6 / FPS, seed=5), 30, 33, quarter-resolution lens, 190 x 338, seed=5): frames,
# then times -- taken at the commit before render grew its flat= argument
RENDER_SHA = ("3bbdf011475101c3e9359c85b5ef4c63e95ca8de1ef92c4fbb10ed53fa4b6a58",
              "458955ce97129c0590366aec3d8fd441ca3017b00fbdfef5d48e3695ac30ecab")


def _small_render(**kw):
    from rssync_amd import synth, synth_video as sv
    g = synth.make_gyro(1.0, 1.0 + 6 / synth.FPS, seed=5)
    return sv.render(g, 30, 33, lens=sv.half_lens(sv.half_lens()), rows=190, cols=338, seed=5, **kw)


def test_render_default_is_unchanged():
    f, t = _small_render()
    assert f.shape == (3, 190, 338)
    assert (hashlib.sha256(f.tobytes()).hexdigest(), hashlib.sha256(t.tobytes()).hexdigest()) == RENDER_SHA


def test_render_flat_region_and_its_mask():
    from rssync_amd import synth_video as sv
    plain, t0 = _small_render()
    region = ((-7.0, -7.0, -7.0), (7.0, -2.0, 7.0))      # the box below y = -2: about half of this view
    f, t, mask = _small_render(flat=region)
    np.testing.assert_array_equal(t, t0)
    assert mask.shape == f.shape and mask.dtype == bool
    assert 0.3 < mask.mean() < 0.7
    assert (f[mask] == sv.FLAT_GRAY).all()
    # elsewhere the same texture, apart from the band around the region where it fades in
    near = mask.copy()
    for _ in range(48):
        near[:, 1:] |= near[:, :-1].copy()
        near[:, :-1] |= near[:, 1:].copy()
        near[:, :, 1:] |= near[:, :, :-1].copy()
        near[:, :, :-1] |= near[:, :, 1:].copy()
    np.testing.assert_array_equal(f[~near], plain[~near])
    assert (f[~mask] == plain[~mask]).mean() > 0.6
    # the region and its complement in the box split the view: every pixel sees exactly one of them
    _, _, other = _small_render(flat=((-7.0, -2.0, -7.0), (7.0, 7.0, 7.0)))
    assert (mask ^ other).all()
    # the detector finds nothing inside the flat part (a feature's 5 x 5 window and its gradients reach 3 px)
    for k in range(f.shape[0]):
        for x, y in fr.detect(f[k], cell=16):
            assert not mask[k, y - 3:y + 4, x - 3:x + 4].all(), (k, x, y)
