"""Gyro conditioning on the device (DESIGN.md section 3 "Gyro conditioning"): raw rates -> uniform grid -> zero-phase
Butterworth -> decimation -> fixed-rate integration -> uniform setter, against the sequential numpy restatement of the
reference's second route (tests/gyro_signal_reference.py: core_support/signal.cpp:3-31, :53-85, core_testcode.cpp:26-34).

Bounds.  Grid, rate, first timestamp: equal.  Rates without a filter: bit-equal (the interpolation is one restated
expression per sample).  Filtered rates: within CHUNKED_R x e_seq of the long-double filter, e_seq being the sequential
fp64 filter's own largest error against it on the same input (measured per case here; CHUNKED_R and how it was measured:
tests/test_gyro_conditioning_cpu.py).  Orientations: the bound of the live rates route (tests/test_gpu_gyro.py: 2e-13, the
same scan) plus, with a filter, CHUNKED_R x e_seq x the stream's length in seconds (a rate error integrated: an angle)."""
import os

import numpy as np
import pytest

import rssync_amd
from rssync_amd import synth

import gyro_signal_reference as ref

pytestmark = pytest.mark.gpu

SEED = 5
DIVIDERS = (0, 3, 32, 256)
DECIMATE = (1, 2, 8)
COMBOS = [(d, k) for d in DIVIDERS for k in DECIMATE if k == 1 or d >= 2 * k]   # what the checks allow
SCAN_ATOL = 2e-13        # tests/test_gpu_gyro.py:107


def stream(n, fs, seed):
    """n samples of a jittered rate stream from t = 0 (synth.make_timestamped's times; the rates of the nominal samples)"""
    g = synth.make_gyro(1.0, 1.0 + max(n / fs - 2.0, 0.01) + 2.0 / fs, fs=fs, seed=seed)
    ts_us, _ = synth.make_timestamped(g, seed=seed)
    assert ts_us.size >= n
    t = ts_us[:n] * 1e-6
    assert np.all(np.diff(t) >= 0)
    return t, np.ascontiguousarray(g.rates[:n])


_cache = {}


def reference(key, t, rates, divider):
    """-> sr, grid times, grid rates (fp64), filtered (sequential fp64), filtered (long double, same coefficients), e_seq"""
    if (key, divider) not in _cache:
        if (key, 0) not in _cache:
            sr, t_new, grid = ref.gyro_interpolate(t, rates)
            _cache[(key, 0)] = (sr, t_new, grid, grid, grid, 0.0)
        sr, t_new, grid = _cache[(key, 0)][:3]
        if divider:
            seq = ref.gyro_lowpass(grid, divider)
            truth = ref.gyro_lowpass(grid, divider, np.longdouble, coef=ref.lowpass_coef(divider))
            _cache[(key, divider)] = (sr, t_new, grid, seq, truth, float(np.max(np.abs(seq - truth))))
    return _cache[(key, divider)]


def check_conditioned(key, t, rates, knots_too):
    for divider, k in COMBOS:
        sr, t_new, grid, seq, truth, e_seq = reference(key, t, rates, divider)
        m_out = grid.shape[0] // k
        h = rssync_amd.SyncProblem(verbose=False)
        h.set_gyro_conditioning(divider, k)
        if m_out < 3:
            with pytest.raises(rssync_amd.RsSyncError, match="fewer than 3 grid samples"):
                h.set_gyro_rates(t, rates)
            continue
        h.set_gyro_rates(t, rates)
        got, fs, t0 = h.gyro_conditioned()
        assert got.shape == (m_out, 3), (key, divider, k)
        assert fs == sr / k and t0 == t_new[0] + (k - 1) / (2.0 * sr), (key, divider, k, fs, t0)
        assert h.gyro_info() == (fs, t0, m_out)
        if divider == 0:
            np.testing.assert_array_equal(got, ref.gyro_decimate(grid, k), err_msg=str((key, divider, k)))
            rate_bound = 0.0
        else:
            err = float(np.max(np.abs(got - np.asarray(ref.gyro_decimate(truth, k)))))
            print("%s divider %d k %d: e_seq %.3g, device error %.3g (ratio %.2f)" % (key, divider, k, e_seq, err, err / e_seq if e_seq else 0.0))
            if grid.shape[0] < 5:       # (nothing is filtered below five samples: both passes only copy)
                np.testing.assert_array_equal(got, ref.gyro_decimate(grid, k))
            assert err <= ref.CHUNKED_R * e_seq, (key, divider, k, err, e_seq)
            rate_bound = ref.CHUNKED_R * e_seq
        if knots_too:
            want = ref.integrate(ref.gyro_decimate(seq, k), k, sr)
            length = m_out * k / sr
            np.testing.assert_allclose(h.gyro_knots(), want, rtol=0, atol=SCAN_ATOL + rate_bound * length,
                                       err_msg=str((key, divider, k)))


@pytest.mark.parametrize("fs", [400.0, 8000.0])
@pytest.mark.parametrize("n", [3, 4, 5, 7, 1000, 5003])
def test_conditioned_rates_and_orientations_match_the_restatement_short(n, fs):
    t, r = stream(n, fs, seed=n)
    check_conditioned(("short", n, fs), t, r, knots_too=True)


def test_conditioned_rates_and_orientations_over_more_than_one_scan_segment():
    """70 001 samples at 8 kHz: three segments of the filter (32 768 samples each) and, undecimated, of the quaternion scan"""
    t, r = stream(70001, 8000.0, seed=7)
    check_conditioned(("mid", 70001), t, r, knots_too=True)


def test_conditioned_rates_of_a_long_log():
    """2^21 + 5 samples at 8 kHz (262 s): 65 segments"""
    n = 2 ** 21 + 5
    t, r = stream(n, 8000.0, seed=9)
    check_conditioned(("long", n), t, r, knots_too=False)


def test_400_hz_over_more_than_one_scan_segment():
    t, r = stream(40001, 400.0, seed=3)
    check_conditioned(("mid400", 40001), t, r, knots_too=False)


def test_complaints_under_conditioning():
    h = rssync_amd.SyncProblem(verbose=False)
    h.set_gyro_conditioning(32, 8)
    t, r = stream(1000, 8000.0, seed=1)
    bad_t = t.copy()
    bad_t[500], bad_t[501] = t[501] + 1e-5, t[500]
    with pytest.raises(rssync_amd.RsSyncError, match="timestamps out of order at pos 501"):
        h.set_gyro_rates(bad_t, r)
    bad_r = r.copy()
    bad_r[17, 1] = np.nan
    with pytest.raises(rssync_amd.RsSyncError, match="non-finite numbers"):
        h.set_gyro_rates(t, bad_r)
    with pytest.raises(rssync_amd.RsSyncError, match="fewer than 3 grid samples"):
        h.set_gyro_rates(t[:20], r[:20])
    for args, msg in (((2, 0), "lowpass_divider 2"), ((0, 65), "decimate must be"), ((8, 8), "needs lowpass_divider >= 16")):
        with pytest.raises(rssync_amd.RsSyncError, match=msg):
            h.set_gyro_conditioning(*args)
    h.set_gyro_rates(t, r)                      # the setting survived the refused ones, and the object is usable
    assert h.gyro_info()[0] == 1000.0


def test_orientation_sweep_under_conditioning():
    """all 48 strings: the sweep's pipeline == set_gyro_rates + PreSync per string == the loop (RSSYNC_SWEEP_PIPELINE=0),
    exactly; the true orientation ranks first; the stream is conditioned once (the same array after every orientation)"""
    F, N = 16, 200
    g = synth.make_gyro(1.0, 1.0 + (F + 2) / synth.FPS, fs=8000.0, seed=77)
    frames = list(synth.make_frames(g, 30, 30 + F, N, seed=77))
    names = list(synth.ORIENTATIONS)
    seq, bat = rssync_amd.SyncProblem(seed=SEED), rssync_amd.SyncProblem(seed=SEED)
    for p in (seq, bat):
        p.set_gyro_conditioning(32, 8)
        for fr in frames:
            p.SetTrackResult(*fr)
    want, first = [], None
    for name in names:
        seq.set_gyro_rates(g.times, g.rates, name)
        cond = seq.gyro_conditioned()
        if first is None:
            first = cond
        np.testing.assert_array_equal(cond[0], first[0])
        assert cond[1:] == first[1:] == (1000.0, first[2])
        want.append(seq.PreSync(0.0, 30, 30 + F, 0.004, 0.1))
    costs, delays = bat.orientation_sweep(g.times, g.rates, names, 0.0, 30, 30 + F, 0.004, 0.1)
    np.testing.assert_array_equal(costs, [w[0] for w in want])
    np.testing.assert_array_equal(delays, [w[1] for w in want])
    np.testing.assert_array_equal(bat.gyro_conditioned()[0], first[0])
    order = np.argsort(costs)
    assert names[order[0]] == "XYZ" and abs(delays[order[0]] - synth.D_TRUE) <= 0.004
    np.testing.assert_array_equal(bat.gyro_knots(), seq.gyro_knots())   # the last orientation stays installed
    os.environ["RSSYNC_SWEEP_PIPELINE"] = "0"
    try:
        costs0, delays0 = bat.orientation_sweep(g.times, g.rates, names, 0.0, 30, 30 + F, 0.004, 0.1)
    finally:
        del os.environ["RSSYNC_SWEEP_PIPELINE"]
    np.testing.assert_array_equal(costs0, costs)
    np.testing.assert_array_equal(delays0, delays)
    # the permutation commutes with the conditioning: the knots of "yXz" are those of the permuted stream under "XYZ"
    a, b = rssync_amd.SyncProblem(seed=SEED), rssync_amd.SyncProblem(seed=SEED)
    for p in (a, b):
        p.set_gyro_conditioning(32, 8)
    a.set_gyro_rates(g.times, g.rates, "yXz")
    b.set_gyro_rates(g.times, synth.orient_rates(g.rates, "yXz"), "XYZ")
    np.testing.assert_array_equal(a.gyro_knots(), b.gyro_knots())


def clean_scene():
    """tests/test_gyro_conditioning_cpu.py's scene: 8 kHz gyro, 32 noise-free frames of 128 tracks"""
    F, N = 32, 128
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, fs=8000.0, seed=2)
    return F, gyro, list(synth.make_frames(gyro, 0, F, N, seed=2, noise=0.0, outliers=0.0))


def test_the_delay_is_not_moved():
    F, gyro, frames = clean_scene()
    raw = rssync_amd.SyncProblem(seed=2, max_outer_iters=150)
    cond = rssync_amd.SyncProblem(seed=2, max_outer_iters=150)
    raw.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)        # every sample a knot
    cond.set_gyro_conditioning(32, 8)
    cond.set_gyro_rates(gyro.times, gyro.rates)
    assert cond.gyro_info()[0] == 1000.0
    out = []
    for p in (raw, cond):
        for fr in frames:
            p.SetTrackResult(*fr)
        _, d0 = p.PreSync(0.0, 0, F, 0.001, 0.08)
        out.append((d0, p.Sync(d0, 0, F, 0.0, 0.08)[1]))
    print("raw (PreSync, Sync) %r, conditioned %r, difference %.3g s" % (out[0], out[1], out[1][1] - out[0][1]))
    assert out[0][0] == out[1][0]                               # the same grid index
    assert abs(out[0][1] - out[1][1]) <= 1e-4
    assert abs(out[0][1] - synth.D_TRUE) <= 1e-4 and abs(out[1][1] - synth.D_TRUE) <= 1e-4


def windows_of(n_tracks, conditioned, F=6):
    g = synth.make_gyro(1.0, 1.0 + (F + 2) / synth.FPS, fs=8000.0, seed=31)
    p = rssync_amd.SyncProblem(seed=SEED, max_outer_iters=5)
    if conditioned:
        p.set_gyro_conditioning(32, 8)
    p.set_gyro_rates(g.times, g.rates)
    for fr in synth.make_frames(g, 30, 30 + F, n_tracks, seed=31):
        p.SetTrackResult(*fr)
    p.PreSync(0.0, 30, 30 + F, 0.001, 0.05)
    p.Sync(synth.D_TRUE, 30, 30 + F, 0.0, 0.05)
    return p.window_info()


def test_a_conditioned_8_khz_log_is_back_on_the_compiled_in_windows():
    raw, cond = windows_of(2048, False), windows_of(2048, True)
    print("2048 tracks: raw %r\n             conditioned %r" % (raw, cond))
    assert raw["presync_window_dynamic"] and not cond["presync_window_dynamic"]
    assert cond["frame_span_knots"] <= 48                       # a pair spans 44 knots of the 80 compiled in
    raw, cond = windows_of(130, False), windows_of(130, True)
    print("130 tracks: raw %r\n            conditioned %r" % (raw, cond))
    # frame_span_knots = floor(t_max) - floor(t_min) + 2 (window_plan.hpp: frame_span): the knots a pair TOUCHES, two more
    # than the knot intervals it is long.  It is the length that shrinks with the rate, to within a knot: 355 -> 45.
    assert abs((cond["frame_span_knots"] - 2) - (raw["frame_span_knots"] - 2) / 8.0) <= 1.0
    assert cond["fp64_window_knots"] < raw["fp64_window_knots"]


def test_switched_off_again_the_live_route_is_untouched():
    t, r = stream(3000, 8000.0, seed=4)
    p, fresh = rssync_amd.SyncProblem(verbose=False), rssync_amd.SyncProblem(verbose=False)
    p.set_gyro_conditioning(32, 8)
    p.set_gyro_rates(t, r, "yXz")
    assert p.gyro_info()[0] == 1000.0
    p.set_gyro_conditioning(None)
    p.set_gyro_rates(t, r, "yXz")
    fresh.set_gyro_rates(t, r, "yXz")
    assert p.gyro_info() == fresh.gyro_info()
    np.testing.assert_array_equal(p.gyro_knots(), fresh.gyro_knots())
    np.testing.assert_array_equal(p.gyro_table(), fresh.gyro_table())


def test_two_contexts_on_one_gpu_give_the_single_context_bits():
    F, gyro, frames = clean_scene()
    res = []
    for ids in (None, [0, 0]):
        p = rssync_amd.SyncProblem(seed=2, max_outer_iters=40)
        if ids:
            p.set_devices(ids)
        p.set_gyro_conditioning(32, 8)
        for fr in frames:
            p.SetTrackResult(*fr)
        p.set_gyro_rates(gyro.times, gyro.rates, "XYZ")
        pre = p.PreSync(0.0, 0, F, 0.001, 0.08)
        syn = p.Sync(pre[1], 0, F, 0.0, 0.08)
        costs, delays = p.orientation_sweep(gyro.times, gyro.rates, list(synth.ORIENTATIONS[:6]) + ["XYZ"], 0.0, 0, F, 0.002, 0.08)
        res.append((pre, syn, costs, delays, p.gyro_knots(), p.gyro_conditioned()))
    one, two = res
    assert one[0] == two[0] and one[1] == two[1]
    np.testing.assert_array_equal(one[2], two[2])
    np.testing.assert_array_equal(one[3], two[3])
    np.testing.assert_array_equal(one[4], two[4])
    np.testing.assert_array_equal(one[5][0], two[5][0])
    assert one[5][1:] == two[5][1:]
