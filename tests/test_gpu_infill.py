"""The infill on the device (include/rssync_infill.h, csrc/kernels/infill.hpp): against the composition of the existing
rssync_stabilize_frames calls, byte for byte; its anchors, its locality, chunks with halos, memory kinds and pitches, its
errors; and the borrowed pixels against the global-shutter truth, held to the float64 restatement's figures
(tests/infill_reference.py)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)

import infill_reference as ir
import rectify_reference as rr
import stabilize_reference as sr
import zoom_reference as zr

pytestmark = pytest.mark.gpu

W, H = rr.COLS, rr.ROWS
N = len(zr.TIMES)
FILL = 77

# name -> (radius, keywords of the device calls)
CASES = {
    "lens-bilinear": (3, dict(camera=sr.LENS, filter=0)),
    "lens-bicubic": (3, dict(camera=sr.LENS, filter=1)),
    "pinhole-resized-bicubic": (3, dict(camera=sr.PINHOLE, filter=1, out_size=(197, 131), zoom=0.8)),
    "pinhole-small-bilinear": (3, dict(camera=sr.PINHOLE, filter=0, out_size=(29, 37), zoom=0.8)),
    "lens-odd-radius-2": (2, dict(camera=sr.LENS, filter=0, out_size=(197, 331))),
}
FIRST = "lens-bilinear"


@pytest.fixture(scope="module")
def scene(built):
    import rssync_amd
    from rssync_amd import synth
    s = dict(rr.scene())
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(s["gyro"].quats, s["gyro"].fs, s["gyro"].t0)
    s["problem"] = p
    frames = np.random.default_rng(5).integers(0, 256, (N, H, W), dtype=np.uint8)
    frames.setflags(write=False)
    s["noise"] = frames
    targets = p.stabilize_path(zr.TIMES, s["lens"][0], synth.D_TRUE, zr.SIGMA)
    targets.setflags(write=False)
    s["targets"] = targets
    return s


def _outside_mask(p, frame, time, target, lens, **kw):
    """one frame through the existing call with fill 0 and fill 255: the pixels that differ are outside"""
    from rssync_amd import synth
    a, _ = p.stabilize_frames(frame[None], [time], lens, synth.D_TRUE, targets=target[None], fill=0, **kw)
    b, _ = p.stabilize_frames(frame[None], [time], lens, synth.D_TRUE, targets=target[None], fill=255, **kw)
    return a[0], a[0] != b[0]


def compose(p, frames, times, targets, lens, radius, fill, **kw):
    """the header's first consequence, through existing calls -> (frames, n_outside, n_borrowed, donors): donors[f] holds per
    pixel the place of its donor in the order, -1 where it got `fill`; sensitive[f]: pixels seen by both frames of a distance
    pair and by nothing before the pair"""
    n = len(times)
    outs, donors, sensitive = [], [], []
    for f in range(n):
        out = donor = both = None
        k = 0
        for d in range(radius + 1):
            pair = []
            for g in ([f] if d == 0 else [f - d, f + d]):
                if 0 <= g < n:
                    img, outside = _outside_mask(p, frames[g], times[g], targets[f], lens, **kw)
                    if out is None:
                        out = np.full(img.shape, fill, np.uint8)
                        donor = np.full(img.shape, -1, np.int64)
                        both = np.zeros(img.shape, bool)
                    pair.append((k, img, ~outside))
                    k += 1
            if len(pair) == 2:
                both |= (donor < 0) & pair[0][2] & pair[1][2]
            for kk, img, ok in pair:
                new = ok & (donor < 0)
                out[new] = img[new]
                donor[new] = kk
        assert k == len(ir.candidates(f, n, radius))
        outs.append(out)
        donors.append(donor)
        sensitive.append(both)
    n_outside = np.array([(d < 0).sum() for d in donors], np.uint64)
    n_borrowed = np.array([(d > 0).sum() for d in donors], np.uint64)
    return np.stack(outs), n_outside, n_borrowed, donors, sensitive


_CACHE = {}


def _case(scene, name):
    """-> (device result, composition) of a case, computed once (read-only)"""
    from rssync_amd import synth
    if name not in _CACHE:
        radius, kw = CASES[name]
        p = scene["problem"]
        got = p.stabilize_frames_infilled(scene["noise"], zr.TIMES, scene["lens"], synth.D_TRUE, radius, targets=scene["targets"], fill=FILL, **kw)
        want = compose(p, scene["noise"], zr.TIMES, scene["targets"], scene["lens"], radius, FILL, **kw)
        for a in got + want[:3]:
            a.setflags(write=False)
        _CACHE[name] = (got, want)
    return _CACHE[name]


def _same(got, want):
    np.testing.assert_array_equal(got[0].cpu().numpy() if isinstance(got[0], torch.Tensor) else got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_composition_byte_for_byte(scene, name):
    got, want = _case(scene, name)
    radius, kw = CASES[name]
    out, n_outside, n_borrowed = got
    print(name, "outside", n_outside.tolist(), "borrowed", n_borrowed.tolist())
    assert out.dtype == np.uint8 and n_outside.dtype == np.uint64 and n_borrowed.dtype == np.uint64
    _same(got, want)
    if name == FIRST:       # from the device-derived masks: the case is not vacuous
        donors, sensitive = want[3], want[4]
        for f in range(N):
            hist = [int((donors[f] == k).sum()) for k in range(len(ir.candidates(f, N, radius)))]
            print(f, hist, int((donors[f] < 0).sum()), int(sensitive[f].sum()))
            assert min(hist) >= 1, (f, hist)
            assert (donors[f] < 0).any(), f
        assert sum(int(s.sum()) for s in sensitive) >= 1


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("explicit", [False, True], ids=["path", "targets"])
@pytest.mark.parametrize("filter", [0, 1], ids=["bilinear", "bicubic"])
def test_radius_zero_and_a_single_frame_are_the_stabiliser(scene, explicit, filter):
    from rssync_amd import synth
    p, frames, lens = scene["problem"], scene["noise"], scene["lens"]
    kw = dict(sigma=zr.SIGMA, fill=FILL, filter=filter)
    want, want_n = p.stabilize_frames(frames, zr.TIMES, lens, synth.D_TRUE, targets=scene["targets"] if explicit else None, **kw)
    assert want_n.sum() > 0
    got, n, nb = p.stabilize_frames_infilled(frames, zr.TIMES, lens, synth.D_TRUE, 0, targets=scene["targets"] if explicit else None, **kw)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(n, want_n)
    assert (nb == 0).all()
    for f in (0, 5):
        t = scene["targets"][f:f + 1] if explicit else None
        got, n, nb = p.stabilize_frames_infilled(frames[f:f + 1], zr.TIMES[f:f + 1], lens, synth.D_TRUE, 3, targets=t, **kw)
        np.testing.assert_array_equal(got[0], want[f])
        assert n[0] == want_n[f] and nb[0] == 0


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_along_the_path_own_pixels_stay_and_the_counts_add_up(scene):
    from rssync_amd import synth
    p, frames, lens = scene["problem"], scene["noise"], scene["lens"]
    base0, base_n = p.stabilize_frames(frames, zr.TIMES, lens, synth.D_TRUE, sigma=zr.SIGMA, fill=0)
    base255, _ = p.stabilize_frames(frames, zr.TIMES, lens, synth.D_TRUE, sigma=zr.SIGMA, fill=255)
    own = base0 == base255
    got, n, nb = p.stabilize_frames_infilled(frames, zr.TIMES, lens, synth.D_TRUE, 3, sigma=zr.SIGMA, fill=FILL)
    print("outside", base_n.tolist(), "still filled", n.tolist(), "borrowed", nb.tolist())
    np.testing.assert_array_equal(got[own], base0[own])
    np.testing.assert_array_equal(n + nb, base_n)
    assert (nb > 0).all()


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 4, 8])
def test_a_frame_depends_on_its_neighbourhood_alone(scene, f):
    from rssync_amd import synth
    (out, n, nb), _ = _case(scene, FIRST)
    lo, hi = max(0, f - 3), min(N - 1, f + 3)
    sub = slice(lo, hi + 1)
    got, gn, gnb = scene["problem"].stabilize_frames_infilled(scene["noise"][sub], zr.TIMES[sub], scene["lens"], synth.D_TRUE, 3,
                                                              targets=scene["targets"][sub], fill=FILL)
    np.testing.assert_array_equal(got[f - lo], out[f])
    assert gn[f - lo] == n[f] and gnb[f - lo] == nb[f]


# 5 ---------------------------------------------------------------------------------------------------------------------
def _per_frame(radius):
    return (2 * radius + 1) * (H + 1) * 36 + 2 * H * W


@pytest.mark.parametrize("budget", [2 * (6 * H * W + 1.5 * _per_frame(3)), 2 * (6 * H * W + 2.5 * _per_frame(3)), 1000],
                         ids=["one-and-a-half-frames", "two-and-a-half-frames", "less-than-a-frame"])
def test_chunks_with_halos(scene, budget):
    from rssync_amd import synth
    got = scene["problem"].stabilize_frames_infilled_budget(scene["noise"], zr.TIMES, scene["lens"], synth.D_TRUE, 3, budget,
                                                            targets=scene["targets"], fill=FILL)
    _same(got, _case(scene, FIRST)[0])


def test_pitched_views_and_device_memory(scene):
    from rssync_amd import synth
    p, frames, lens = scene["problem"], scene["noise"], scene["lens"]
    want = _case(scene, FIRST)[0]
    kw = dict(targets=scene["targets"], fill=FILL)
    # device-resident tensors
    dev = torch.from_numpy(np.array(frames)).to("cuda:0")
    got = p.stabilize_frames_infilled(dev, zr.TIMES, lens, synth.D_TRUE, 3, **kw)
    assert isinstance(got[0], torch.Tensor) and got[0].is_cuda
    _same(got, want)
    # host in, device out
    dout = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda:0")
    got = p.stabilize_frames_infilled(frames, zr.TIMES, lens, synth.D_TRUE, 3, out=dout, **kw)
    assert got[0] is dout
    _same(got, want)
    # pitched device buffers, a guard pattern between the rows of the result
    wide = np.zeros((N, H + 2, W + 61), np.uint8)
    wide[:, 1:1 + H, 13:13 + W] = frames
    dwide = torch.from_numpy(wide).to("cuda:0")
    dout = torch.full((N, H + 3, W + 19), 201, dtype=torch.uint8, device="cuda:0")
    view = dout[:, 2:2 + H, 3:3 + W]
    res, n, nb = p.stabilize_frames_infilled(dwide[:, 1:1 + H, 13:13 + W], zr.TIMES, lens, synth.D_TRUE, 3, out=view, **kw)
    assert res is view
    back = dout.cpu().numpy()
    _same((back[:, 2:2 + H, 3:3 + W], n, nb), want)
    guard = np.ones(back.shape, bool)
    guard[:, 2:2 + H, 3:3 + W] = False
    assert (back[guard] == 201).all()
    # pitched host buffers, the same way
    hout = np.full((N, H + 1, W + 5), 9, np.uint8)
    _, n, nb = p.stabilize_frames_infilled(wide[:, 1:1 + H, 13:13 + W], zr.TIMES, lens, synth.D_TRUE, 3, out=hout[:, :H, 2:2 + W], **kw)
    _same((hout[:, :H, 2:2 + W], n, nb), want)
    assert (hout[:, H:] == 9).all() and (hout[:, :, :2] == 9).all() and (hout[:, :, 2 + W:] == 9).all()


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_and_the_next_call_works(scene):
    from rssync_amd import infill, stabilize, synth
    p, frames, lens = scene["problem"], np.ascontiguousarray(scene["noise"]), scene["lens"]
    want = _case(scene, FIRST)[0]
    lib = infill.library()
    lib.rssync_set_panic_mode(1)
    PD, PU64 = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    L = np.ascontiguousarray(lens, np.float64)
    T = np.ascontiguousarray(zr.TIMES)
    Q = np.ascontiguousarray(scene["targets"])
    prm = stabilize.params(fill=FILL)
    res = np.zeros_like(frames)
    n, nb = np.zeros(N, np.uint64), np.zeros(N, np.uint64)

    def call(f=frames.ctypes.data, t=T, delay=synth.D_TRUE, o=None, radius=3):
        o = res.ctypes.data if o is None else o
        return lib.rssync_infill_stabilize(p._h, f, N, W, H, W, W * H, None if t is None else t.ctypes.data_as(PD), L.ctypes.data, delay,
                                           Q.ctypes.data_as(PD), C.byref(prm), o if o else None, W, H, W, W * H, n.ctypes.data_as(PU64),
                                           radius, nb.ctypes.data_as(PU64))

    late = T.copy()
    late[6] = 9.0
    for match, kw in (("radius", dict(radius=-1)), ("radius", dict(radius=9)), ("no frames", dict(f=None)), ("null output", dict(o=0)),
                      ("no frame times", dict(t=None)), ("overlaps", dict(o=frames.ctypes.data + W * H)),
                      ("leaves the gyro data", dict(t=late))):
        assert call(**kw) != 0, kw
        msg = lib.rssync_last_error().decode()
        assert match in msg and msg.startswith(("infill: ", "stabilize: ")), (match, msg)
        assert call() == 0, lib.rssync_last_error().decode()
        _same((res, n, nb), want)
    assert call(radius=8) == 0 and call(radius=0) == 0
    with pytest.raises(infill.RsSyncError, match="radius"):
        p.stabilize_frames_infilled(frames, zr.TIMES, lens, synth.D_TRUE, 9)


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_borrowed_pixels_against_the_global_shutter_truth(scene):
    """Mean absolute grey difference to sr.truth() over the pixels the device borrowed, frames 32, 33, 34: at most the
    float64 restatement's ir.BORROWED_ERROR plus ir.ERROR_MARGIN; at least 99 % of the outside pixels borrowed; the own
    pixels within the stabiliser's bound."""
    from rssync_amd import synth
    p, lens = scene["problem"], scene["lens"]
    frames, times = ir.video()
    targets = ir.video_targets()
    kw = dict(targets=targets)
    own0, own_n = p.stabilize_frames(frames, times, lens, synth.D_TRUE, fill=0, **kw)
    own255, _ = p.stabilize_frames(frames, times, lens, synth.D_TRUE, fill=255, **kw)
    out, n, nb = p.stabilize_frames_infilled(frames, times, lens, synth.D_TRUE, ir.RADIUS, fill=0, **kw)
    out255, _, _ = p.stabilize_frames_infilled(frames, times, lens, synth.D_TRUE, ir.RADIUS, fill=255, **kw)
    truth = sr.truth()
    for k, f in enumerate(range(*ir.VIDEO_SCENE.indices(len(times)))):
        outside = own0[f] != own255[f]
        lent = outside & (out[f] == out255[f])
        assert outside.sum() == own_n[f] and lent.sum() == nb[f] and own_n[f] == n[f] + nb[f]
        err = float(np.abs(out[f].astype(np.float64) - truth[k].astype(np.float64))[lent].mean())
        own = rr.grey_error(out[f], truth[k], ~outside)
        share = float(nb[f]) / float(own_n[f])
        print("frame %d: %d of %d outside pixels borrowed (%.4f; reference %d of %d), error %.3f (reference %.3f, fill %.1f), own %.4f "
              "(reference %.4f)" % (rr.F0 + k, nb[f], own_n[f], share, ir.SEEN[k], ir.OUTSIDE[k], err, ir.BORROWED_ERROR[k],
                                    ir.FILL_ERROR[k], own, sr.REFERENCE_ERROR[k]))
        assert err <= ir.BORROWED_ERROR[k] + ir.ERROR_MARGIN, (k, err)
        assert share >= ir.MIN_BORROWED_SHARE, (k, share)
        assert own <= 1.05 * sr.REFERENCE_ERROR[k], (k, own)
