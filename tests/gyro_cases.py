"""Named gyro rate streams that a real log produces and synth.make_gyro does not: a camera that stands still, a
saturated or spinning sensor, repeated timestamps, dropouts, bursts, and a time base far from 0.  Data only: nothing
here touches the library.  Shared by tests/test_gyro_cases_cpu.py (which proves that every stream reaches the branch it
is there for) and tests/test_gpu_gyro_hostile.py (which runs them on the device).

    case        content                                                              what it is there to reach
    still       all rates exactly 0                                                  gyro_delta's else-branch; slerp of equal
                                                                                     neighbours (dot >= 1: acos 0 or NaN -> lerp)
    deadband    make_gyro, first 2 s exactly 0, components below 0.05 rad/s -> 0     the same inside a moving stream
    tiny        rates of 1e-170 / 1e-160 mixed into a normal stream                  th2 underflows to 0 while w != 0
    saturated   make_gyro x 40, clipped to +-34.9 rad/s per axis                     plateaus with step edges; the scan at speed
    spin        250 rad/s about (2, -1, 3) / sqrt(14), jittered timestamps           a closed form at 0.6 rad per sample
    flip        50 Hz, 175 rad/s about the same axis: 3.5 rad per sample             neighbour dot = cos 1.75 < 0: slerp's sign flip
    repeats     every 7th timestamp equals the one before it, rates differ;          dt == 0; interpolation on duplicates and on
                every 200th sample on its nominal time                               grid points that sit on a sample
    dropouts    gaps of 0.05 s, 0.5 s and 2 s in a 400 Hz stream                     n / span rounds to another multiple of 50 Hz
    bursts      16 samples 10 us apart, then a pause of 16 nominal intervals         dt of 10 us beside dt of 2 ms (8 kHz nominal)

Every case is ``make(name, n, t0_s, seed) -> (times_s, rates)``, deterministic.  ``t0_s`` is a whole number of seconds
added to every timestamp: whole seconds move the integer-microsecond grid by a whole number of samples."""
import numpy as np

from rssync_amd import synth

N_DEFAULT = 5003
# lengths at which gyro_scan_kernel's chunks (ceil(n / 1024) samples for each of 1024 threads), its idle threads, the
# number of 32 768-sample segments and the last segment's total change shape; 32 769 and 98 305 leave a last segment of one
EDGES = (1023, 1024, 1025, 32767, 32768, 32769, 65536, 65537, 98305)
# 200 000 s at the 7400 Hz that `bursts` rounds to: first grid sample 1.48e9, below 2^31
T0S = (0, 3600, 65536, 200000)
NAMES = ("still", "deadband", "tiny", "saturated", "spin", "flip", "repeats", "dropouts", "bursts")

FIRST = 1.0                 # every stream starts one second after its time base (timestamps must not be negative)
AXIS = np.array([2.0, -1.0, 3.0]) / np.sqrt(14.0)
SATURATION = 34.9           # 2000 deg/s
DROPOUTS = ((0.2, 0.05), (0.5, 0.5), (0.8, 2.0))     # (where, as a fraction of the stream; seconds lost)


def _rates(n, fs, seed):
    """n samples of synth.make_gyro's rates (2 rad/s sinusoids plus noise) at fs"""
    g = synth.make_gyro(FIRST, FIRST + n / fs, fs=fs, seed=seed, margin=2.0 / fs)
    assert g.rates.shape[0] >= n
    return np.ascontiguousarray(g.rates[:n])


def _jittered(n, fs, seed, jitter=0.2):
    """nominal sample times moved by up to +-jitter of one interval; strictly increasing"""
    rng = np.random.default_rng([seed, 17])
    t = FIRST + (np.arange(n) + rng.uniform(-jitter, jitter, n)) / fs
    assert np.all(np.diff(t) > 0)
    return t


def still(n, seed):
    return _jittered(n, 400.0, seed), np.zeros((n, 3))


def deadband(n, seed):
    t, r = _jittered(n, 400.0, seed), _rates(n, 400.0, seed)
    r[t < FIRST + 2.0] = 0.0
    r[np.abs(r) < 0.05] = 0.0
    return t, r


def tiny(n, seed):
    t, r = _jittered(n, 400.0, seed), _rates(n, 400.0, seed)
    r[3::5] = [1e-170, -1e-160, 1e-170]        # (w * dt)^2 is below the smallest subnormal: th2 == 0, w != 0
    r[4::25] = [0.0, 1e-160, 0.0]
    return t, r


def saturated(n, seed):
    return _jittered(n, 400.0, seed), np.clip(_rates(n, 400.0, seed) * 40.0, -SATURATION, SATURATION)


def spin(n, seed):
    return _jittered(n, 400.0, seed), np.tile(250.0 * AXIS, (n, 1))


def flip(n, seed):
    # +-3 % of an interval at either end: 3.5 rad +- 0.21 per sample, half of it stays between 1.64 and 1.86 (pi / 2 = 1.57)
    return _jittered(n, 50.0, seed, jitter=0.03), np.tile(175.0 * AXIS, (n, 1))


def repeats(n, seed):
    t, r = _jittered(n, 400.0, seed), _rates(n, 400.0, seed)
    t[6::7] = t[5::7][:t[6::7].size]
    for i in range(0, n, 200):                  # whole and half seconds: samples that sit exactly on a grid point
        if i % 7 not in (5, 6):
            t[i] = FIRST + i / 400.0
    assert np.all(np.diff(t) >= 0) and np.all(np.any(r[6::7] != r[5::7][:r[6::7].shape[0]], axis=1))
    return t, r


def without_dropouts(n, seed):
    return _jittered(n, 400.0, seed), _rates(n, 400.0, seed)


def dropouts(n, seed):
    t, r = without_dropouts(n, seed)
    t = t.copy()
    for where, gap in DROPOUTS:
        t[int(where * n):] += gap
    return t, r


def bursts(n, seed):
    fs, per = 8000.0, 16
    i = np.arange(n)
    t = FIRST + (i // per) * (per * 10e-6 + per / fs) + (i % per) * 10e-6
    rng = np.random.default_rng([seed, 23])
    t = t + rng.uniform(-2e-6, 2e-6, n)         # the samples of a burst stay 6 .. 14 us apart
    assert np.all(np.diff(t) > 0)
    return t, _rates(n, fs, seed)


_MAKERS = dict(still=still, deadband=deadband, tiny=tiny, saturated=saturated, spin=spin, flip=flip, repeats=repeats,
               dropouts=dropouts, bursts=bursts)
_cache = {}


def make(name, n=N_DEFAULT, t0_s=0, seed=None):
    """-> (times_s [n], rates [n][3]), fresh copies.  The seed defaults to one per (case, length)."""
    assert t0_s == int(t0_s)
    if seed is None:
        seed = 1000 * NAMES.index(name) + n % 997
    key = (name, n, seed)
    if key not in _cache:
        _cache[key] = _MAKERS[name](n, seed)
    t, r = _cache[key]
    return t + float(t0_s), r.copy()


def timestamps_us(t):
    """core_testcode.cpp:48-50: whole microseconds by truncation, in fp64"""
    return (np.asarray(t, np.float64) * 1000000).astype(np.int64)


def constant(n=N_DEFAULT, seed=3):
    """rates (0.3, -0.2, 0.1) throughout, jittered timestamps: what a low-pass must hand through"""
    return _jittered(n, 400.0, seed), np.tile([0.3, -0.2, 0.1], (n, 1))


ORIENTATIONS = (None, "yXz")


def runs():
    """every (case, length, time base, orientation) of the rates route that the device tests run: all cases at the
    default length over every time base and both orientations, and `saturated` at the scan's edge lengths, the time
    bases taken in turn"""
    out = [(name, N_DEFAULT, t0, o) for name in NAMES for t0 in T0S for o in ORIENTATIONS]
    out += [("saturated", n, T0S[i % len(T0S)], None) for i, n in enumerate(EDGES)]
    return out


def run_id(run):
    return "%s-%d-t%d-%s" % (run[0], run[1], run[2], run[3] or "XYZ")
