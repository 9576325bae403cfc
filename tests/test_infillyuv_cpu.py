"""The infill for 4:2:2 and 4:4:4 video without a GPU: its numpy restatement (tests/infillyuv_reference.py) against its
recorded figures, the chunk plan of a three-plane 4:2:2 call with a halo and one table region (csrc/frame_plan.hpp, compiled
as tests/test_frame_plan.py compiles it), the public header as C99, and what the built library exports and holds."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import infill_reference as ir
import infillyuv_reference as iyr
import test_frame_plan as tfp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


# the restatement ---------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_its_recorded_figures():
    """every figure of infillyuv_reference.py's table, computed here: the outside and the seen chroma samples at both sitings,
    the errors of U and V at CENTER, and the share of the outside samples that a candidate within radius 3 sees"""
    fig = iyr.figures()
    for plane in (0, 1):
        for k, (outside, seen, err, fill_err, near) in enumerate(fig[plane]):
            print(plane, k, outside, seen, round(err, 3), round(fill_err, 1), near, round(iyr.error_margin(k), 3))
            assert (outside, seen, near) == (iyr.OUTSIDE[iyr.CENTER][k], iyr.SEEN[iyr.CENTER][k], iyr.NEAR_EDGE[k])
            assert round(err, 3) == iyr.BORROWED_ERROR[plane][k] and round(fill_err, 1) == iyr.FILL_ERROR[plane][k]
            assert seen / outside >= iyr.MIN_BORROWED_SHARE
            assert err <= iyr.FAR_BELOW * fill_err
            assert 0 < iyr.error_margin(k) < 1.0            # grey levels: the bound of the device test says something
    left = iyr.counts(iyr.LEFT)
    print(left)
    assert tuple(o for o, _ in left) == iyr.OUTSIDE[iyr.LEFT] and tuple(s for _, s in left) == iyr.SEEN[iyr.LEFT]
    assert all(s / o >= iyr.MIN_BORROWED_SHARE for o, s in left)
    # the counts as first computed, spelled out: a changed table above fails here too
    assert iyr.OUTSIDE == {iyr.CENTER: (4614, 5193, 4699), iyr.LEFT: (4610, 5189, 4695)}
    assert iyr.SEEN == {iyr.CENTER: (4608, 5193, 4695), iyr.LEFT: (4604, 5189, 4691)}
    assert iyr.MIN_BORROWED_SHARE == ir.MIN_BORROWED_SHARE


def test_chroma_placement_is_the_gray_placement_with_the_chroma_camera():
    """frame 33: several candidates of the order are first hits of chroma samples, the histogram adds up to the recorded
    counts, and a donor's position is inside the 380 x 338 chroma plane"""
    _, _, _, times = iyr.video()
    f = 3
    place, pos, _ = iyr.chroma_hits(f)
    cand = ir.candidates(f, len(times), iyr.RADIUS)
    hist, left = ir.histogram(place, len(cand))
    print(cand, hist, left)
    assert place.shape == (380, 338) and sum(hist) + left == place.size
    assert cand == [3, 2, 4, 1, 5, 0, 6] and hist[0] > 0.9 * place.size and sum(h > 0 for h in hist[1:]) >= 3
    assert sum(hist[1:]) == iyr.SEEN[iyr.CENTER][1] and sum(hist[1:]) + left == iyr.OUTSIDE[iyr.CENTER][1]
    assert np.isnan(pos[place < 0]).all() and np.isfinite(pos[place >= 0]).all()
    ok = place >= 0
    assert (pos[ok][:, 0] >= 0).all() and (pos[ok][:, 0] <= 337).all() and (pos[ok][:, 1] >= 0).all() and (pos[ok][:, 1] <= 379).all()


# the chunk plan ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("infillyuv_plan")
    src = d / "shim.cpp"
    src.write_text(tfp.SHIM)
    out = d / "libframeplan.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "rs-sync_amd", "csrc"),
                           "-o", str(out), str(src)])
    L = ctypes.CDLL(str(out))
    UL = ctypes.POINTER(ctypes.c_ulong)
    L.plan.argtypes = [ctypes.c_uint, ctypes.c_ulong, UL, ctypes.c_uint, ctypes.c_uint, ctypes.c_int, UL, ctypes.c_int, UL, UL]
    return L


@pytest.mark.parametrize("n_frames", [1, 2, 5, 7, 9, 100])
@pytest.mark.parametrize("size", [(3, 4), (31, 38), (199, 330), (380, 676)])
def test_plan_of_a_three_plane_422_call_with_one_table_region_and_a_halo(plan_lib, size, n_frames):
    """I422 through rship_infillyuv_frames at radius 3: tabs = 7 tables of the one region per frame (the chroma plane reads
    the luma's), three planes in and out, the chroma planes as high as the luma"""
    rows, cols = size
    radius, tabs = 3, 7
    tab = (tfp.tab_bytes(rows), 0)
    planes = [(cols, rows), (cols // 2, rows), (cols // 2, rows)]
    image = sum(rb * r for rb, r in planes)
    per_frame = tabs * sum(tab) + 2 * image
    halo = min(2 * radius, n_frames - 1) * image
    chunks = set()
    for budget in [1000, 2 * (halo + per_frame), 2 * (halo + 2.5 * per_frame), 2 * (halo + 4.5 * per_frame), 2 * (halo + 20 * per_frame), 0]:
        for pin, pout in ((planes, planes), ([], planes), (planes, []), ([], [])):
            p = tfp.plan(plan_lib, n_frames, budget, tab, pin, pout, tables=tabs, radius=radius)
            chunk = p["chunk"]
            chunks.add(chunk)
            assert 1 <= chunk <= n_frames
            assert p["held"] == min(n_frames, chunk + 2 * radius)
            assert p["two_slots"] == (n_frames > chunk)
            # the regions in the layout's order: the tables, input planes (held frames), output planes (chunk frames)
            regions = [(p["off_tab"][0], chunk * tabs * tab[0])]
            regions += [(p["off_in"][k], p["held"] * rb * r) for k, (rb, r) in enumerate(pin)]
            regions += [(p["off_out"][k], chunk * rb * r) for k, (rb, r) in enumerate(pout)]
            end = 0
            for off, nbytes in regions:
                assert off >= end
                end = off + nbytes
            assert end <= p["slot_bytes"]
            assert p["off_tab"][0] == 0
            if chunk > 1:       # (a chunk of one frame is the least there is, whatever the budget)
                half = (budget if budget else tfp.DEFAULT_BUDGET) // 2
                assert p["slot_bytes"] <= half + 2 * 255, (p, half)
    if n_frames == 9 and size == (380, 676):      # the budgets of tests/test_gpu_infillyuv.py give the chunks it names
        got = [tfp.plan(plan_lib, 9, b, tab, planes, planes, tables=tabs, radius=radius)["chunk"]
               for b in (1000, 2 * (halo + 2.5 * per_frame), 2 * (halo + 4.5 * per_frame))]
        assert got == [1, 2, 4]
    assert 1 in chunks


# the header and the library ----------------------------------------------------------------------------------------------
def test_public_header_is_c99(tmp_path):
    src = tmp_path / "infillyuv.c"
    src.write_text('#include "rssync_infillyuv.h"\n'
                   'int main(void) { return RSSYNC_INFILL_MAX_RADIUS == 8 && RSSYNC_YUV_I410 == 51 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o",
                    str(tmp_path / "infillyuv.o"), str(src)], check=True)


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


CF = [(c, f) for c in (0, 1) for f in (0, 1)]
LEND_KERNELS = (["lend422_8_kernelILi%dELb%dELi%dEE" % (c, nv, f) for c, f in CF for nv in (0, 1)]
                + ["lend422_16_kernelILi%dELb%dELi%dELi%dEE" % (c, semi, sh, f) for c, f in CF for semi, sh in ((1, 6), (1, 0), (0, 0))]
                + ["lend444_8_kernelILi%dELi%dEE" % cf for cf in CF]
                + ["lend444_16_kernelILi%dELi%dEE" % cf for cf in CF])
# what the tests of the other families count their kernels by
OTHER_FAMILIES = ("donor", "infill", "stabilize", "rectify", "zoom", "bicubic", "limit_", "color_", "color16_", "percam_", "framecam_")
YUV_FAMILY = re.compile(r"yuv4(22|44)(_16)?_kernel")


def test_library_exports_the_infill_and_holds_its_kernels(built, tmp_path):
    import rssync_amd
    from rssync_amd import infillyuv
    lib = rssync_amd.library_path()
    text = open(os.path.join(ROOT, "include", "rssync_infillyuv.h")).read()
    declared = set(re.findall(r"\b(rssync_infillyuv_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == {"rssync_infillyuv_stabilize"}
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {e for e in exported if e.startswith("rssync_infillyuv")} == declared
    assert {e for e in exported if e.startswith("rship_infillyuv")} == {"rship_infillyuv_frames"}
    assert {s for s in infillyuv.SIGNATURES if s.startswith("rssync_")} == declared and "rship_infillyuv_frames" in infillyuv.SIGNATURES
    infillyuv.library()                 # binds every signature: a missing symbol raises
    for name in ("stabilize_yuv_infilled", "stabilize_yuv_infilled_budget"):
        assert callable(getattr(rssync_amd.SyncProblem, name)) and callable(getattr(infillyuv, name))
    # the code object: every kernel of the family is there, once, and needs neither scratch nor spills
    assert len(LEND_KERNELS) == 28 and len(set(LEND_KERNELS)) == 28
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "lend4" in name.lower():
            found[name] = {k: int(re.search(r"\.%s:\s+(\S+)" % k, block).group(1))
                           for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    for want in LEND_KERNELS:
        hit = [n for n in found if want in n]
        assert len(hit) == 1, (want, sorted(found))
        print(want, found[hit[0]])
    assert len(found) == len(LEND_KERNELS), sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        # the kernel's name and its argument struct's, which is part of it: of no family that other tests count
        assert not any(fam in name.lower() for fam in OTHER_FAMILIES), name
        assert not YUV_FAMILY.search(name.lower()), name
