"""The colour infill without a GPU: its numpy restatement (tests/colorinfill_reference.py) against its recorded figures, the
chunk plan of a three-plane call with a halo (csrc/frame_plan.hpp, compiled as tests/test_frame_plan.py compiles it), the
public header as C99, and what the built library exports and holds."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import colorinfill_reference as cir
import infill_reference as ir
import test_frame_plan as tfp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


# the restatement ---------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_its_recorded_figures():
    """every figure of colorinfill_reference.py's table, computed here: the luma rows are infill_reference's (the same
    camera), and the share of the outside chroma samples that a candidate within radius 3 sees reaches the recorded bound"""
    fig = cir.figures()
    for plane in (0, 1, 2):
        for k, (outside, seen, err, fill_err, near) in enumerate(fig[plane]):
            print(plane, k, outside, seen, round(err, 3), round(fill_err, 1), near, round(cir.error_margin(plane, k), 3))
            assert (outside, seen, near) == (cir.OUTSIDE[plane][k], cir.SEEN[plane][k], cir.NEAR_EDGE[plane][k])
            assert round(err, 3) == cir.BORROWED_ERROR[plane][k] and round(fill_err, 1) == cir.FILL_ERROR[plane][k]
            assert seen / outside >= cir.MIN_BORROWED_SHARE[plane]
            assert err <= cir.FAR_BELOW * fill_err
            assert 0 < cir.error_margin(plane, k) < 1.0         # grey levels: the bound of the device test says something
    assert cir.OUTSIDE[0] == ir.OUTSIDE and cir.SEEN[0] == ir.SEEN
    assert cir.BORROWED_ERROR[0] == ir.BORROWED_ERROR and cir.FILL_ERROR[0] == ir.FILL_ERROR
    assert cir.OUTSIDE[1] == cir.OUTSIDE[2] and cir.SEEN[1] == cir.SEEN[2]      # U and V: one position, one donor


def test_chroma_placement_is_the_gray_placement_with_the_chroma_camera():
    """frame 33: several candidates of the order are first hits of chroma samples, the histogram adds up to the recorded
    counts, and a donor's position is inside the chroma plane"""
    _, _, _, times = cir.video()
    f = 3
    place, pos, _ = cir.chroma_hits(f)
    cand = ir.candidates(f, len(times), cir.RADIUS)
    hist, left = ir.histogram(place, len(cand))
    print(cand, hist, left)
    assert place.shape == (190, 338) and sum(hist) + left == place.size
    assert cand == [3, 2, 4, 1, 5, 0, 6] and hist[0] > 0.9 * place.size and sum(h > 0 for h in hist[1:]) >= 3
    assert sum(hist[1:]) == cir.SEEN[1][1] and sum(hist[1:]) + left == cir.OUTSIDE[1][1]
    assert np.isnan(pos[place < 0]).all() and np.isfinite(pos[place >= 0]).all()
    ok = place >= 0
    assert (pos[ok][:, 0] >= 0).all() and (pos[ok][:, 0] <= 337).all() and (pos[ok][:, 1] >= 0).all() and (pos[ok][:, 1] <= 189).all()


# the chunk plan ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("colorinfill_plan")
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
@pytest.mark.parametrize("size", [(38, 30), (330, 198), (380, 676)])
def test_plan_of_a_three_plane_call_with_two_table_regions_and_a_halo(plan_lib, size, n_frames):
    """I420 through rship_colorinfill_frames at radius 3: tabs = 7 tables of each region per frame, three planes in and out"""
    rows, cols = size
    radius, tabs = 3, 7
    tab = (tfp.tab_bytes(rows), tfp.tab_bytes(rows // 2))
    planes = [(cols, rows), (cols // 2, rows // 2), (cols // 2, rows // 2)]
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
            # the regions in the layout's order: tables, input planes (held frames), output planes (chunk frames)
            regions = [(p["off_tab"][i], chunk * tabs * tab[i]) for i in range(2)]
            regions += [(p["off_in"][k], p["held"] * rb * r) for k, (rb, r) in enumerate(pin)]
            regions += [(p["off_out"][k], chunk * rb * r) for k, (rb, r) in enumerate(pout)]
            end = 0
            for off, nbytes in regions:
                assert off >= end
                end = off + nbytes
            assert end <= p["slot_bytes"]
            assert p["off_tab"][0] == 0 and p["off_tab"][1] % 256 == 0
            if chunk > 1:       # (a chunk of one frame is the least there is, whatever the budget)
                half = (budget if budget else tfp.DEFAULT_BUDGET) // 2
                assert p["slot_bytes"] <= half + 2 * 255, (p, half)
    if n_frames == 9 and size == (380, 676):      # the budgets of tests/test_gpu_colorinfill.py give the chunks it names
        got = [tfp.plan(plan_lib, 9, b, tab, planes, planes, tables=tabs, radius=radius)["chunk"]
               for b in (1000, 2 * (halo + 2.5 * per_frame), 2 * (halo + 4.5 * per_frame))]
        assert got == [1, 2, 4]
    assert 1 in chunks


# the header and the library ----------------------------------------------------------------------------------------------
def test_public_header_is_c99(tmp_path):
    src = tmp_path / "colorinfill.c"
    src.write_text('#include "rssync_colorinfill.h"\n'
                   'int main(void) { return RSSYNC_INFILL_MAX_RADIUS == 8 && RSSYNC_COLOR16_I010 == 19 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o",
                    str(tmp_path / "colorinfill.o"), str(src)], check=True)


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip("no %s in this image" % path)
    return path


CF = [(c, f) for c in (0, 1) for f in (0, 1)]
DONOR_KERNELS = (["donor_rows_kernel"]
                 + ["donor_yuv8_kernelILi%dELb%dELi%dEE" % (c, nv, f) for c, f in CF for nv in (0, 1)]
                 + ["donor_yuv16_kernelILi%dELb%dELi%dELi%dEE" % (c, semi, sh, f) for c, f in CF for semi, sh in ((1, 6), (1, 0), (0, 0))]
                 + ["donor_rgba8_kernelILi%dELi%dEE" % cf for cf in CF]
                 + ["donor_gray16_kernelILi%dELi%dEE" % cf for cf in CF])
OTHER_FAMILIES = ("infill", "stabilize", "rectify", "zoom", "bicubic", "limit_", "color_", "color16_", "percam_")


def test_library_exports_the_colour_infill_and_holds_its_kernels(built, tmp_path):
    import rssync_amd
    from rssync_amd import colorinfill
    lib = rssync_amd.library_path()
    text = open(os.path.join(ROOT, "include", "rssync_colorinfill.h")).read()
    declared = set(re.findall(r"\b(rssync_colorinfill_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == {"rssync_colorinfill_stabilize"}
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {e for e in exported if e.startswith("rssync_colorinfill")} == declared
    assert {e for e in exported if e.startswith("rship_colorinfill")} == {"rship_colorinfill_frames"}
    assert {s for s in colorinfill.SIGNATURES if s.startswith("rssync_")} == declared and "rship_colorinfill_frames" in colorinfill.SIGNATURES
    colorinfill.library()               # binds every signature: a missing symbol raises
    for name in ("stabilize_color_infilled", "stabilize_color_infilled_budget"):
        assert callable(getattr(rssync_amd.SyncProblem, name)) and callable(getattr(colorinfill, name))
    # the code object: every kernel of the family is there, once, and needs neither scratch nor spills
    assert len(DONOR_KERNELS) == 29 and len(set(DONOR_KERNELS)) == 29
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "copy.so")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "donor" in name.lower():
            found[name] = {k: int(re.search(r"\.%s:\s+(\S+)" % k, block).group(1))
                           for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    for want in DONOR_KERNELS:
        hit = [n for n in found if want in n]
        assert len(hit) == 1, (want, sorted(found))
        print(want, found[hit[0]])
    assert len(found) == len(DONOR_KERNELS), sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        # the kernel's name and its argument struct's, which is part of it: of no family that other tests count
        assert not any(fam in name.lower() for fam in OTHER_FAMILIES), name
