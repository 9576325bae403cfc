"""The host arithmetic that cuts a call of a frame front door into chunks and lays a chunk slot out (rs-sync_amd/csrc/
frame_plan.hpp; rssync_kernels.hip's frame_pipeline runs the plan).  It is plain C++ without HIP, so it is compiled here
with g++ behind a one-function C shim and checked on the CPU: the budgets of the GPU tests give the chunks their
docstrings promise, the regions of a slot never overlap, and without a halo the numbers are the closed formulas."""
import ctypes
import itertools
import os
import subprocess

import pytest

import rectify_reference as rr
import zoom_reference as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = r'''
#include "frame_plan.hpp"
// tab[2]; in, out: {row_bytes, rows} per plane -> res: chunk, held, two_slots, slot_bytes, off_tab[2], off_in[3], off_out[3]
extern "C" void plan(unsigned n_frames, unsigned long budget, const unsigned long* tab, unsigned tabs, unsigned radius, int n_in,
                     const unsigned long* in, int n_out, const unsigned long* out, unsigned long* res) {
    rs::FrameLayout q;
    q.n_frames = n_frames;
    q.budget = budget;
    q.tab[0] = tab[0];
    q.tab[1] = tab[1];
    q.tabs = tabs;
    q.radius = radius;
    q.n_in = n_in;
    q.n_out = n_out;
    for (int k = 0; k < n_in; ++k) q.in[k] = {in[2 * k], (uint32_t)in[2 * k + 1]};
    for (int k = 0; k < n_out; ++k) q.out[k] = {out[2 * k], (uint32_t)out[2 * k + 1]};
    const rs::FramePlan p = rs::plan_frames(q);
    res[0] = p.chunk; res[1] = p.held; res[2] = p.two_slots; res[3] = p.slot_bytes;
    for (int i = 0; i < 2; ++i) res[4 + i] = p.off_tab[i];
    for (int k = 0; k < 3; ++k) { res[6 + k] = p.off_in[k]; res[9 + k] = p.off_out[k]; }
}
extern "C" unsigned long default_budget() { return rs::kRectBudget; }
extern "C" unsigned max_chunk() { return rs::kRectMaxChunk; }
'''
DEFAULT_BUDGET, MAX_CHUNK = 256 << 20, 32768     # the issue's numbers: 0 means 256 MiB, a chunk is the grid's z


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_plan")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    out = d / "libframeplan.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "rs-sync_amd", "csrc"),
                           "-o", str(out), str(src)])
    L = ctypes.CDLL(str(out))
    UL = ctypes.POINTER(ctypes.c_ulong)
    L.plan.argtypes = [ctypes.c_uint, ctypes.c_ulong, UL, ctypes.c_uint, ctypes.c_uint, ctypes.c_int, UL, ctypes.c_int, UL, UL]
    L.default_budget.restype = ctypes.c_ulong
    return L


def plan(L, n_frames, budget, tabs, planes_in, planes_out, tables=1, radius=0):
    """tabs: bytes of a table per region (1 or 2); planes_*: [(row_bytes, rows)], [] = device memory -> dict"""
    tab = (ctypes.c_ulong * 2)(*(list(tabs) + [0])[:2])
    flat = lambda pl: (ctypes.c_ulong * 6)(*([v for p in pl for v in p] + [0] * 6)[:6])   # noqa: E731
    res = (ctypes.c_ulong * 12)()
    L.plan(n_frames, int(budget), tab, tables, radius, len(planes_in), flat(planes_in), len(planes_out), flat(planes_out), res)
    r = [int(v) for v in res]
    return dict(chunk=r[0], held=r[1], two_slots=bool(r[2]), slot_bytes=r[3], off_tab=r[4:6], off_in=r[6:9], off_out=r[9:12])


def tab_bytes(rows):
    return (rows + 1) * 9 * 4


def chunk_sizes(n_frames, chunk):
    return [min(chunk, n_frames - f0) for f0 in range(0, n_frames, chunk)]


def test_the_constants(lib):
    assert lib.default_budget() == DEFAULT_BUDGET and lib.max_chunk() == MAX_CHUNK


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_the_gpu_tests_budgets_give_the_chunks_their_docstrings_promise(lib):
    R, Cc, orows, ocols, n = rr.ROWS, rr.COLS, 200, 320, rr.N_FRAMES
    assert n == 3
    # test_gpu_stabilize.py: one and a half frames per slot, three chunks of one frame
    per_frame = (R + 1) * 36 + R * Cc + orows * ocols
    p = plan(lib, n, 2 * 1.5 * per_frame, [tab_bytes(R)], [(Cc, R)], [(ocols, orows)])
    assert chunk_sizes(n, p["chunk"]) == [1, 1, 1] and p["two_slots"]
    # test_gpu_color.py: NV12, both tables and one and a half planes a side
    per_frame = (R + 1) * 36 + (R // 2 + 1) * 36 + R * Cc * 3 // 2 + orows * ocols * 3 // 2
    nv12 = lambda w, h, b=1: [(b * w, h), (b * w, h // 2)]   # noqa: E731
    p = plan(lib, n, 2 * 1.5 * per_frame, [tab_bytes(R), tab_bytes(R // 2)], nv12(Cc, R), nv12(ocols, orows))
    assert chunk_sizes(n, p["chunk"]) == [1, 1, 1] and p["two_slots"]
    # test_gpu_color16.py: P010, a frame costs twice the 8-bit bytes
    per_frame = (R + 1) * 36 + (R // 2 + 1) * 36 + 2 * (R * Cc * 3 // 2) + 2 * (orows * ocols * 3 // 2)
    p = plan(lib, n, 2 * 1.5 * per_frame, [tab_bytes(R), tab_bytes(R // 2)], nv12(Cc, R, 2), nv12(ocols, orows, 2))
    assert chunk_sizes(n, p["chunk"]) == [1, 1, 1] and p["two_slots"]
    # test_gpu_rectify.py: seven 37 x 29 frames, two and a half frames per slot: four chunks
    rows, cols = 37, 29
    per_frame = (rows + 1) * 36 + 2 * rows * cols
    p = plan(lib, 7, 2 * 2.5 * per_frame, [tab_bytes(rows)], [(cols, rows)], [(cols, rows)])
    assert chunk_sizes(7, p["chunk"]) == [2, 2, 2, 1] and p["two_slots"]


@pytest.mark.parametrize("frames_per_slot,chunk", [(1.5, 1), (2.5, 2), (None, 1)], ids=["one-and-a-half-frames", "two-and-a-half-frames", "less-than-a-frame"])
def test_infills_budgets_at_radius_3(lib, frames_per_slot, chunk):
    """test_gpu_infill.py's three budgets: a slot pays for the halo's six input frames before it pays for a frame"""
    H, W, N, radius = rr.ROWS, rr.COLS, len(zr.TIMES), 3
    per_frame = (2 * radius + 1) * (H + 1) * 36 + 2 * H * W
    budget = 1000 if frames_per_slot is None else 2 * (6 * H * W + frames_per_slot * per_frame)
    p = plan(lib, N, budget, [tab_bytes(H)], [(W, H)], [(W, H)], tables=2 * radius + 1, radius=radius)
    assert p["chunk"] == chunk and p["held"] == min(N, chunk + 6) and p["two_slots"] == (N > chunk)


# 2, 3 ------------------------------------------------------------------------------------------------------------------
def _planes(n, w, h):
    """1: gray or RGBA-like; 2: NV12-like; 3: I420-like"""
    return {1: [(w, h)], 2: [(w, h), (w, h // 2)], 3: [(w, h), (w // 2, h // 2), (w // 2, h // 2)]}[n]


def test_the_regions_of_a_slot_do_not_overlap_and_the_chunk_is_in_range(lib):
    sizes = [(2, 2), (3, 2), (2, 3), (7, 5), (16, 9), (29, 37), (40, 40), (39, 40), (40, 39)]      # width, height: 2 .. 40, odd and even
    budgets = [1, 255, 4096, 70000, 1 << 20, 0]                                                    # (0: the default)
    checked = 0
    for (w, h), n_planes, n_tabs, radius, dev_in, dev_out, budget in itertools.product(sizes, (1, 2, 3), (1, 2), range(9), (False, True),
                                                                                         (False, True), budgets):
        ow, oh = w + 3, h + 1
        tabs = [tab_bytes(h), tab_bytes(h // 2)][:n_tabs]
        pin = [] if dev_in else _planes(n_planes, w, h)
        pout = [] if dev_out else _planes(n_planes, ow, oh)
        places = 2 * radius + 1
        for n_frames in (1, 2, 5, 40, 100000):
            p = plan(lib, n_frames, budget, tabs, pin, pout, tables=places, radius=radius)
            chunk, held = p["chunk"], p["held"]
            assert 1 <= chunk <= min(n_frames, MAX_CHUNK)
            assert p["two_slots"] == (n_frames > chunk)
            assert held == min(n_frames, chunk + 2 * radius)
            regions = [(p["off_tab"][i], chunk * places * t) for i, t in enumerate(tabs)]
            regions += [(p["off_in"][k], held * rb * rows) for k, (rb, rows) in enumerate(pin)]
            regions += [(p["off_out"][k], chunk * rb * rows) for k, (rb, rows) in enumerate(pout)]
            for off, _ in regions[:n_tabs]:
                assert off % 256 == 0
            end = 0
            for off, size in regions:       # in the layout's order: tables, input planes, output planes
                assert off >= end
                end = off + size
            assert end <= p["slot_bytes"]
            checked += 1
    assert checked == len(sizes) * 3 * 2 * 9 * 2 * 2 * len(budgets) * 5


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_without_a_halo_the_values_are_the_closed_formulas(lib):
    """chunk = min(min(n_frames, 32768), max(1, budget / 2 / per_frame)); each table region's bytes rounded up to 256; then
    the input planes [chunk][rows][row_bytes], then the output planes"""
    up = lambda v: (v + 255) // 256 * 256   # noqa: E731
    for (w, h), n_planes, n_tabs, dev_in, dev_out, budget, n_frames in itertools.product(
            [(2, 2), (7, 5), (29, 37), (40, 39), (676, 380)], (1, 2, 3), (1, 2), (False, True), (False, True), [1, 4096, 70000, 3 << 20, 0],
            (1, 3, 7, 100000)):
        ow, oh = w + 3, h + 1
        tabs = [tab_bytes(h), tab_bytes(h // 2)][:n_tabs]
        pin = [] if dev_in else _planes(n_planes, w, h)
        pout = [] if dev_out else _planes(n_planes, ow, oh)
        per_frame = sum(tabs) + sum(rb * r for rb, r in pin) + sum(rb * r for rb, r in pout)
        chunk = min(min(n_frames, 32768), max(1, (budget or DEFAULT_BUDGET) // 2 // per_frame))
        want_tab, off = [0, 0], 0
        for i in range(2):
            want_tab[i] = off
            off += up(chunk * tabs[i]) if i < n_tabs else 0
        want_in, want_out = [0, 0, 0], [0, 0, 0]
        for k, (rb, r) in enumerate(pin):
            want_in[k] = off
            off += chunk * rb * r
        for k, (rb, r) in enumerate(pout):
            want_out[k] = off
            off += chunk * rb * r
        p = plan(lib, n_frames, budget, tabs, pin, pout)
        assert p == dict(chunk=chunk, held=chunk, two_slots=n_frames > chunk, slot_bytes=off, off_tab=want_tab, off_in=want_in, off_out=want_out)
