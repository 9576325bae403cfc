"""The pixel front door -- rssync_ext_set_track_pixels -> pack_frames_kernel's pixel branch (csrc/kernels/support.hpp,
csrc/lens_math.hpp) -- across lenses, image edges, frame sizes, mixed packs, row times where rounding shows, and the
non-finite counter.  Every check is a function of a `make` factory: it runs on the CPU stand-in (tests/cpu_device, the same
lens_math.hpp text compiled with g++) and, marked gpu, on the device.  The reference side is always the oracle fed the
driver's way (oracle.pixels_to_tracks, then SetTrackResult), never the library.  Helpers: tests/pixel_cases.py.

tests/measure/gpu_pixel_front_door.py writes what the device measures to profiles/pixel_front_door.json; the caps asserted are
the project's existing ones (1.2e-7 per fp32 component, 1 % of components differing in any bit, 1e-13 on fp64 rows of P),
not measured figures."""
import numpy as np
import pytest

import pixel_cases as pc

SEED, LENSES = pc.SEED, pc.LENSES
COUNTS = (10000, 1, 8193, 2, 63, 8192, 64, 2049, 65, 255, 2048, 256, 513, 257, 512)   # one frame each, in this order
BIT_SHARE_CAP = 0.01    # the project's cap on fp32 components that differ in any bit (test_upstream_steps.py)


def _host(hosttest_lib):
    import rssync_amd
    return lambda **kw: rssync_amd.SyncProblem(seed=SEED, _lib=hosttest_lib, **kw)


def _device():
    import torch  # noqa: F401  (imported before the library: torch ships its own HIP runtime, tests/test_gpu_parity.py)
    import rssync_amd
    return lambda **kw: rssync_amd.SyncProblem(seed=SEED, **kw)


# ---- 1-3: lenses x point sets, both stream sets ----------------------------------------------------------------------
def _check_lens(make, name, share_cap):
    """One problem per lens, one frame per point set (uniform inside; corners, edge midpoints, (0, 0) at A / B / both, the
    principal point and its neighbours; a margin of half an image; both sides of the model's range).  fp32 streams within
    1.2e-7 of the oracle-fed twin and the time columns bit-equal EVERYWHERE; fp64 rows within 1e-13 of the oracle and of the
    library fed the oracle's rays on the in-image tracks; the share of in-image components that differ in any bit.
    CPU stand-in: the share is 0 for every lens (asserted), the largest fp32 difference anywhere 1.1e-13, the fp64 rows
    within 9.3e-16 of the oracle and 8.3e-16 of the ray-fed library.  Device: the cap stays the project's 1 %; the
    device's own shares and largest differences per lens are the content of profiles/pixel_front_door.json, written by
    tests/measure/gpu_pixel_front_door.py."""
    t = pc.check_lens(make, name, seed=11)
    print("lens %-8s in-image fp32 components differing: %d of %d (share %.2e); max fp32 diff %.3g; P64 vs oracle %.3g, "
          "vs ray-fed %.3g" % (name, t.diff, t.total, t.share(), t.max32, t.max64_oracle, t.max64_rays))
    assert t.total > 8000
    assert t.share() <= share_cap, (name, t.diff, t.total)
    return t


@pytest.mark.parametrize("name", LENSES)
def test_lens_on_the_host_solver(hosttest_lib, built, name):
    _check_lens(_host(hosttest_lib), name, 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LENSES)
def test_lens_on_the_device(built, name):
    _check_lens(_device(), name, BIT_SHARE_CAP)


def test_point_sets_reach_the_halving_loop(built):
    """the screen for 'stop the halving loop after one trip': in every lens' straddle set (and in the margin set of every
    lens whose range ends inside the margin) some points need two or more trips of lens_math.hpp's halving loop while others
    in the same wave of 64 need none"""
    for name, (lens, cols, rows) in pc.lenses().items():
        sets = {k: (a, b) for k, a, b in pc.point_sets(lens, cols, rows, 11)}
        mixed = 0
        for key in ("straddle", "margin"):
            trips = pc.halving_trips(lens, sets[key][0])
            assert trips.max() >= 2 or key == "margin", (name, key)
            w = trips[:len(trips) // 64 * 64].reshape(-1, 64)
            mixed += int(((w.max(axis=1) >= 2) & (w.min(axis=1) == 0)).sum())
        assert mixed > 0, name


def _check_nonmonotonic(make):
    """k1 = -0.3 alone: the model has no inverse over most of the image, and two correct restatements of the reference's
    schedule (Horner form here, expanded powers in the oracle) end up to 4.2e-7 apart on the CPU already -- finite garbage
    on both sides.  So no parity is claimed: the call returns, every ray is finite and of unit norm, PreSync runs."""
    from rssync_amd import synth
    lens = pc.nonmonotonic_lens()
    gyro = synth.make_gyro(0.0, 8 / synth.FPS, seed=5)
    rng = np.random.default_rng(5)
    p = make()
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    for fr in range(6):
        pa, pb = pc._uniform(rng, 300, pc.COLS, pc.ROWS, 0.25), pc._uniform(rng, 300, pc.COLS, pc.ROWS, 0.25)
        p.set_track_pixels(fr, fr / synth.FPS, (fr + 1) / synth.FPS, pa, pb, lens, pc.ROWS)
    for fr in range(6):
        a, b = p.frame_rays(fr)
        assert np.isfinite(a).all() and np.isfinite(b).all()
        na = np.sqrt(a[:, 0].astype(np.float64) ** 2 + a[:, 2].astype(np.float64) ** 2 + b[:, 0].astype(np.float64) ** 2)
        nb = np.sqrt(a[:, 1].astype(np.float64) ** 2 + a[:, 3].astype(np.float64) ** 2 + b[:, 1].astype(np.float64) ** 2)
        assert np.abs(na - 1).max() <= 1e-6 and np.abs(nb - 1).max() <= 1e-6
    c, d = p.PreSync(0.0, 0, 6, 0.004, 0.05)
    assert np.isfinite(c) and np.isfinite(d)


def test_nonmonotonic_lens_on_the_host_solver(hosttest_lib, built):
    _check_nonmonotonic(_host(hosttest_lib))


@pytest.mark.gpu
def test_nonmonotonic_lens_on_the_device(built):
    _check_nonmonotonic(_device())


# ---- 4: counts and layout -----------------------------------------------------------------------------------------------
def _check_counts(make, share_cap):
    """One problem holding a frame of each of 1 .. 10000 tracks (the kernel's blockIdx.y loop, the 256-thread block edges,
    the classes above 2048 and 8192 tracks), anisotropic lens, every row its own random point, the last row of each
    frame the far corner: streams and fp64 rows of every frame as in the lens check."""
    from rssync_amd import synth
    lens, cols, rows = pc.lenses()["aniso"]
    rng = np.random.default_rng(17)
    frames = []
    for i, n in enumerate(COUNTS):
        pa, pb = pc._uniform(rng, n, cols, rows), pc._uniform(rng, n, cols, rows)
        pa[-1], pb[-1] = (cols, rows), (0.0, rows)
        frames.append(pc.frame(i, i / synth.FPS, (i + 1) / synth.FPS, pa, pb, lens, rows, cols))
    gyro = synth.make_gyro(0.0, (len(frames) + 2) / synth.FPS, seed=17)
    hp, hr = pc.feed(make(), gyro, frames, "pixels"), pc.feed(make(), gyro, frames, "oracle")
    o = pc.oracle_problem(gyro, frames, SEED)
    t = pc.Tally()
    for f in frames:
        pc.compare_streams(hp, hr, f, t, gyro)
        pc.compare_p64(hp, hr, o, f, t)
    print("counts: in-image fp32 components differing %d of %d; max fp32 diff %.3g; P64 vs oracle %.3g"
          % (t.diff, t.total, t.max32, t.max64_oracle))
    assert t.total == 8 * sum(COUNTS) and t.share() <= share_cap


def test_counts_on_the_host_solver(hosttest_lib, built):
    _check_counts(_host(hosttest_lib), 0.0)


@pytest.mark.gpu
def test_counts_on_the_device(built):
    _check_counts(_device(), BIT_SHARE_CAP)


MIXED_SIZES = (64, 600, 2100)   # the one-wave kernels, four waves, the class above 2048 tracks
MIXED_ARGS = (0.0, 0, 12, 0.004, 0.1)


def _mixed_frames(swap=None):
    """12 frames: pixel frames of three lenses and two image_rows, ray frames between them.  swap = {frame: (kind, size)}
    replaces one"""
    from rssync_amd import synth
    L = pc.lenses()
    s, m, b = MIXED_SIZES
    plan = [("synth", s), ("rays", s), ("aniso", m), ("half", s), ("rays", m), ("aniso", b), ("half", m), ("rays", b),
            ("synth", m), ("half", b), ("aniso", s), ("synth", b)]
    for fr, spec in (swap or {}).items():
        plan[fr] = spec
    gyro = synth.make_gyro(0.0, (len(plan) + 2) / synth.FPS, seed=23)
    frames = []
    for fr, (kind, n) in enumerate(plan):
        lens, cols, rows = L["aniso" if kind == "rays" else kind]
        _, ta, tb, pa, pb = next(iter(synth.make_pixel_frames(gyro, fr, fr + 1, n, seed=23, lens=lens, rows=rows, cols=cols)))
        frames.append(pc.frame(fr, ta, tb, pa, pb, lens, rows, cols, rays=(kind == "rays")))
    return gyro, frames


def _check_mixed(make, share_cap):
    """Pixel frames of three lenses and two image_rows interleaved with ray frames in one pack (is_pixels is decided per
    block, the lens travels per frame): every frame's streams against the oracle-fed twin, PreSync's delay equal and its
    cost within rel 1e-5.  Then a pixel frame becomes a ray frame and back, and a 64-track frame becomes a 2100-track
    frame (its class changes) and back: each time the streams against the twin again, and streams and PreSync equal to the
    bits of a freshly built problem."""
    gyro, frames = _mixed_frames()
    hp, hr = pc.feed(make(), gyro, frames, "pixels"), pc.feed(make(), gyro, frames, "oracle")
    o = pc.oracle_problem(gyro, frames, SEED)
    t = pc.Tally()

    def compare(frames, hr, o):
        for f in frames:
            pc.compare_streams(hp, hr, f, t, gyro)
            pc.compare_p64(hp, hr, o, f, t, delays=pc.DELAYS[:1])

    compare(frames, hr, o)
    c1, d1 = hp.PreSync(*MIXED_ARGS)
    c2, d2 = hr.PreSync(*MIXED_ARGS)
    assert d1 == d2 and c1 == pytest.approx(c2, rel=1e-5)
    for swap in ({2: ("rays", MIXED_SIZES[1])}, None, {0: ("synth", MIXED_SIZES[2])}, None):
        _, now = _mixed_frames(swap)
        for fr in (swap or last):   # the frames that change: set in the live object, everything else stays
            pc.set_frame(hp, now[fr], "pixels")
        last = swap
        fresh = pc.feed(make(), gyro, now, "pixels")
        twin = pc.feed(make(), gyro, now, "oracle")
        compare(now, twin, pc.oracle_problem(gyro, now, SEED))
        pc.same_streams(hp, fresh, now)
        assert hp.PreSync(*MIXED_ARGS) == fresh.PreSync(*MIXED_ARGS)
    assert hp.PreSync(*MIXED_ARGS) == (c1, d1)
    print("mixed pack: in-image fp32 components differing %d of %d; max fp32 diff %.3g; P64 vs oracle %.3g"
          % (t.diff, t.total, t.max32, t.max64_oracle))
    assert t.share() <= share_cap


def test_mixed_pack_on_the_host_solver(hosttest_lib, built):
    _check_mixed(_host(hosttest_lib), 0.0)


@pytest.mark.gpu
def test_mixed_pack_on_the_device(built):
    _check_mixed(_device(), BIT_SHARE_CAP)


# ---- 5: row times where rounding shows ---------------------------------------------------------------------------------
ROWTIME_CASES = [(fs, ro, rows) for fs in (400.0, 8000.0) for ro in (0.0, None, 0.033) for rows in (1520, 2160, 760)]


ROWTIME_NEAR = 0.05   # s: frame times where the products are inexact (see the screen below)


def _rowtime_scene(fs, ro, rows, t_begin):
    from rssync_amd import synth
    ro = synth.READOUT if ro is None else ro
    base, cols0, rows0 = pc.lenses()["aniso"]
    lens = pc.with_readout(pc.scaled_lens(base, rows / rows0), ro)
    # (near t = 0 the gyro's time base starts at exactly 0: ts - start is then exact, and ts keeps all its bits)
    gyro = synth.make_gyro(t_begin, t_begin + 0.4, fs=fs, seed=29, margin=0.25 if t_begin > 1 else t_begin)
    return gyro, pc.rowtime_frames(lens, cols0 * rows / rows0, rows, fs, gyro.t0, 29, t_begin=t_begin), lens


def test_rowtime_inputs_make_the_products_inexact(built):
    """The screen the row-time checks rest on, in exact rational arithmetic (pixel_cases.fused_screen): which inputs give
    other bits when knot_offset's (ts - start) * fs - base or row_time's frame_time + ro * (y / rows) is contracted to one
    fused operation.
    Frame times near 3600 s: NO case passes, and none can.  ts and start are multiples of 2^-41 there and less than half a
    second apart, so ts - start has at most 40 significant bits and its product with 400 or 8000 is exact; row_time's
    product is ~1e-5 of the sum, so fusing it changes the sum only within ~1e-24 of a rounding boundary.  Those cases check
    what large times do stress -- the sum's own rounding, ts - start, the base knot -- but prove nothing about contraction.
    Frame times near 0.05 s (gyro from exactly 0 s): ts carries 53 significant bits and ts - start keeps them, so the product
    is inexact.  EVERY case there passes the screen for knot_offset (readout 0 included), and every case with a readout
    passes it for row_time, in the fp64 row times and in the fp32 stream.  _check_rowtimes runs both sets.
    What sees which: the oracle-fed library takes its row times from the oracle's C but its offsets from the same
    rs::knot_offset as the pixel-fed one, so the comparison of the two routes exposes a fused row_time only; a fused
    knot_offset is exposed by the comparison with pixel_cases.restated_offsets, numpy's separately rounded operations."""
    for fs, ro, rows in ROWTIME_CASES:
        gyro, frames, _ = _rowtime_scene(fs, ro, rows, pc.ROWTIME_T0)
        n_knot, n_row32, n_row64, total = pc.fused_screen(frames, gyro.t0, fs)
        assert (n_knot, n_row32, n_row64) == (0, 0, 0), (fs, ro, rows)
        gyro, frames, _ = _rowtime_scene(fs, ro, rows, ROWTIME_NEAR)
        for f in frames[1:]:
            x = (f["ta"] + f["lens"][0] * (f["pa"][:, 1].min() / rows) - gyro.t0) * fs
            assert 0 < x - np.floor(x) < 1e-8
        n_knot, n_row32, n_row64, total = pc.fused_screen(frames, gyro.t0, fs)
        print("t = 0.05 s, fs %5d ro %.5f rows %4d: fused knot_offset moves %d fp32 offsets, fused row_time %d (fp64 row times "
              "%d) of %d" % (fs, frames[0]["lens"][0], rows, n_knot, n_row32, n_row64, total))
        assert n_knot >= 16, (fs, ro, rows)
        assert ro == 0.0 or (n_row64 >= 16 and n_row32 >= 1), (fs, ro, rows)


def _check_rowtimes(make, cases, t_begin):
    """frame times an hour into the gyro's time base and 50 ms into it, 400 Hz and 8 kHz, readouts 0 / 11.11 ms / 33 ms,
    1520 / 2160 / 760 rows, y from a quarter image above to a quarter below: the time columns bit-equal to the oracle-fed
    route AND to the numpy restatement of row_time, base knot and knot_offset (pixel_cases.restated_offsets), again after
    set_readout (the re-timing kernel) against a fresh oracle-fed problem and the restatement with that readout, and the
    fp64 rows within 1e-13 of the oracle."""
    t = pc.Tally()
    for fs, ro, rows in cases:
        gyro, frames, lens = _rowtime_scene(fs, ro, rows, t_begin)
        hp, hr = pc.feed(make(), gyro, frames, "pixels"), pc.feed(make(), gyro, frames, "oracle")
        o = pc.oracle_problem(gyro, frames, SEED)
        rays = []
        for f in frames:
            rays.append(pc.compare_streams(hp, hr, f, t, gyro))
            pc.compare_p64(hp, hr, o, f, t)
        ro2 = 0.02 if lens[0] != 0.02 else 0.01
        hp.set_readout(ro2)
        again = [dict(f, lens=pc.with_readout(f["lens"], ro2)) for f in frames]
        hr2 = pc.feed(make(), gyro, again, "oracle")
        for f, (a0, b0) in zip(again, rays):
            a1, b1 = pc.compare_streams(hp, hr2, f, t, gyro)
            np.testing.assert_array_equal(pc.u32(a1), pc.u32(a0))            # the directions do not depend on the readout
            np.testing.assert_array_equal(pc.u32(b1[:, :2]), pc.u32(b0[:, :2]))
        o2 = pc.oracle_problem(gyro, again, SEED)
        for f in again[:2]:
            pc.compare_p64(hp, hr2, o2, f, t, delays=pc.DELAYS[:1])
    print("row times from t = %g: max fp32 ray diff %.3g; P64 vs oracle %.3g" % (t_begin, t.max32, t.max64_oracle))


def test_rowtimes_on_the_host_solver(hosttest_lib, built):
    _check_rowtimes(_host(hosttest_lib), ROWTIME_CASES, pc.ROWTIME_T0)
    _check_rowtimes(_host(hosttest_lib), ROWTIME_CASES, ROWTIME_NEAR)


@pytest.mark.gpu
def test_rowtimes_on_the_device(built):
    _check_rowtimes(_device(), ROWTIME_CASES, pc.ROWTIME_T0)
    _check_rowtimes(_device(), ROWTIME_CASES, ROWTIME_NEAR)


# ---- 6: the non-finite counter (pixel_cases.check_counter) ----------------------------------------------------------------
def test_counter_on_the_host_solver(hosttest_lib, built):
    assert pc.check_counter(_host(hosttest_lib)) == pc.COUNTER_K


@pytest.mark.gpu
def test_counter_on_the_device(built):
    """K = 1283 (pixel_cases.COUNTER_K); tests/measure/gpu_pixel_front_door.py records the device's K on one context and
    on two in profiles/pixel_front_door.json"""
    assert pc.check_counter(_device()) == pc.COUNTER_K


@pytest.mark.gpu
def test_counter_sums_over_two_contexts(built):
    """the same with the frames spread over two contexts of one object (cut at 64 frames; bad frames on both sides), as
    test_gpu_readout_sweep.py::test_two_contexts_in_one_object_give_the_same_bits spreads them; check_counter asserts
    device_count() == 2"""
    assert pc.check_counter(_device(), contexts=2) == pc.COUNTER_K


# ---- 7: end to end per lens -----------------------------------------------------------------------------------------------
def _check_end_to_end(make, name):
    """A clean pixel scene through a lens other than synth.LENS: PreSync's arg-min equal to the oracle's, Sync within 1e-4 s
    of the true delay and of the oracle.  The oracle alone (CPU, 40 frames x 160 tracks, seed 13) lands 1.37e-5 s (wide) and
    2.51e-5 s (aniso) from the truth: the reference's nine Newton steps with the coefficient 8 on k4 have converged well
    enough over 5..95 % of these images, so both lenses stay in the test."""
    from rssync_amd import synth
    lens, cols, rows = pc.lenses()[name]
    F = 40
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, seed=13)
    frames = [pc.frame(fr, ta, tb, pa, pb, lens, rows, cols) for fr, ta, tb, pa, pb in
              synth.make_pixel_frames(gyro, 0, F, 160, seed=13, noise_px=0.0, outliers=0.0, lens=lens, rows=rows, cols=cols)]
    h = pc.feed(make(), gyro, frames, "pixels")
    o = pc.oracle_problem(gyro, frames, SEED)
    dh = h.PreSync(0.0, 0, F, 0.002, 0.1)[1]
    do = o.PreSync(0.0, 0, F, 0.002, 0.1)[1]
    assert dh == do
    _, dh = h.Sync(dh, 0, F - 1, 0.0, 0.2)
    _, do = o.Sync(do, 0, F - 1, 0.0, 0.2)
    print("end to end, lens %s: Sync %.7f s, oracle %.7f s, truth %.4f s" % (name, dh, do, synth.D_TRUE))
    assert abs(do - synth.D_TRUE) < 1e-4      # the oracle itself: the condition for keeping this lens here
    assert abs(dh - synth.D_TRUE) < 1e-4 and abs(dh - do) < 1e-4


@pytest.mark.parametrize("name", ("wide", "aniso"))
def test_end_to_end_on_the_host_solver(hosttest_lib, built, name):
    _check_end_to_end(_host(hosttest_lib), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("wide", "aniso"))
def test_end_to_end_on_the_device(built, name):
    _check_end_to_end(_device(), name)
