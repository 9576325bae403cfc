"""The association of a window's sum, restated in a few lines, and the windows and scenes of the tests that hold every
route to it (tests/test_window_sums_cpu.py, tests/test_gpu_long_windows.py).

Every per-window number Sync and PreSync decide on -- loss, derivative, the ten line-search trials, a candidate's cost --
is a sum over the window's frames in ONE association (kernels/support.hpp, plan_sum_kernel's comment): the slots are cut
into chunks at the multiples of 64 of the sorted frame table, a chunk is added in slot order, the chunks are added in
order.  plan_sum is that rule in plain float64, one addition at a time; flat_sum and exact_sum are what it is told apart
from.  Nothing here looks at a device; the scenes are plain numpy (rssync_amd.synth).
"""
import functools
import math

import numpy as np

CHUNK = 64          # sync_problem.cpp: kChunk


def plan_sum(values, first_table_index):
    """Sum of a window's per-slot values in the plan's association.  `values[i]` belongs to frame-table index
    `first_table_index + i` (a window is a run of consecutive table indices; with frames 0 .. F-1 all set, the table
    index of a frame is its number).  The chunk rule is apply_selection's (sync_problem.cpp: `block = slots[pos] / kChunk`,
    a new chunk whenever the block changes): a chunk is the window's slots whose TABLE index falls into the same block of
    64 -- so the first chunk of a window that does not begin at a multiple of 64 is ragged, and so is its last.  A chunk
    is added sequentially from 0.0 in slot order, the chunk sums are added sequentially from 0.0 in chunk order."""
    total = 0.0
    acc = 0.0
    block = None
    for i, v in enumerate(values):
        b = (first_table_index + i) // CHUNK
        if b != block:
            if block is not None:
                total = total + acc
            block = b
            acc = 0.0
        acc = acc + float(v)
    if block is not None:
        total = total + acc
    return total


def flat_sum(values):
    """the values added one after the other, no chunks"""
    acc = 0.0
    for v in values:
        acc = acc + float(v)
    return acc


def exact_sum(values):
    """the correctly rounded sum (math.fsum)"""
    return math.fsum(float(v) for v in values)


def n_chunks(begin, length):
    return (begin + length - 1) // CHUNK - begin // CHUNK + 1


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# (begin, length) in frames.  Why these lengths -- rows x slots against the staging areas of the three device routes:
#   64, 65          one chunk / the first window with two
#   129, 641, 1281  first un-staged windows of exec_window_sums (kernels/executor.hpp: rows * n_slots <= 1280) with the
#                   10 trial rows, the 2 loss + derivative rows, the 1 final-loss row
#   205, 1025       first un-staged windows of window_sums (kernels/syncloop.hpp: rows * span <= 2048) with 10 and 2 rows
#   4161            from index 0: 65 full chunks and one slot -- more than 64 chunks, where a thread of plan_sum_kernel
#                   (kernels/support.hpp) takes a second chunk and its thread 0 adds four groups of 16 chunk sums and a tail
#   begin 37, 5     a ragged first chunk;  (63, 2) two one-slot chunks;  (100, 1) a single slot
SMALL_WINDOWS = [(0, 64), (0, 65), (37, 129), (37, 641), (5, 1281), (0, 1400), (63, 2), (100, 1)]     # within 1400 frames
CPU_LOSS_WINDOWS = SMALL_WINDOWS + [(37, 205), (37, 1025), (0, 4161)]
GPU_LOSS_WINDOWS = [(0, 65), (37, 129), (37, 205), (5, 641), (37, 1025), (5, 1281), (0, 4161), (100, 4200)]
PRESYNC_WINDOWS = [(37, 129), (0, 4161), (100, 4200)]
# overlapping windows of one batched PreSync: a frame has a position in several windows, the plan carries an index list
# (plan_sum_kernel's idx != NULL)
PRESYNC_BATCH_BEGINS = [0, 37, 300, 5]
PRESYNC_BATCH_ENDS = [4161, 166, 941, 1286]            # exclusive
SYNC_LENGTHS = [129, 205, 641, 1025, 1281]             # one Sync window each, from frame SYNC_BEGIN
SYNC_BEGIN = 37
# windows of one batched Sync: staged and un-staged ones side by side
SYNC_BATCH_BEGINS = [0, 37, 300, 5, 640]
SYNC_BATCH_ENDS = [39, 165, 940, 1285, 1300]           # inclusive: 40, 129, 641, 1281 and 661 frames
POINTS_WINDOW, POINTS_POSITIONS, POINTS_REPEATS = 200, [0, 150, 411], 2

LOSS_DELAYS = (0.0362, 0.03)
BATCH_DELAYS = (0.0362, 0.0359, 0.0371, 0.05, 0.0362 + 1e-9)
PRESYNC_ARGS = (0.036, 0.002, 0.006)                   # initial delay, step, radius: six candidates


class Scene:
    def __init__(self, gyro, frames):
        self.gyro, self.frames, self.F = gyro, frames, len(frames)

    def fill(self, *problems, begin=0, end=None):
        for p in problems:
            p.SetGyroQuaternions(self.gyro.quats, self.gyro.fs, self.gyro.t0)
            for fr in self.frames[begin:end]:
                p.SetTrackResult(*fr)


@functools.lru_cache(maxsize=None)
def uniform_scene(F, N, seed=5, fs=400.0):
    """F frames from 0 of N tracks each, noisy with 10 % outliers"""
    from rssync_amd import synth
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, fs=fs, seed=seed)
    return Scene(gyro, list(synth.make_frames(gyro, 0, F, N, seed=seed)))


def _per_frame_scene(F, seed, tracks_of):
    from rssync_amd import synth
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, seed=seed)
    rng = np.random.default_rng(seed)
    frames = []
    for fr in range(F):
        frames += list(synth.make_frames(gyro, fr, fr + 1, tracks_of(fr, rng), seed=seed))
    return Scene(gyro, frames)


@functools.lru_cache(maxsize=None)
def ragged_scene(F=1400, seed=21):
    """frames of 2 .. 40 tracks, a 130-track frame every 16th: the kernels' smallest instantiations with ragged tails,
    and a frame that takes the next one"""
    return _per_frame_scene(F, seed, lambda fr, rng: 130 if fr % 16 == 7 else int(rng.integers(2, 41)))


@functools.lru_cache(maxsize=None)
def straggler_scene(F=720, seed=22):
    """every tenth frame has 600 tracks (more than a wave's 512: the executor's BIG instantiation), the rest 16 .. 130"""
    return _per_frame_scene(F, seed, lambda fr, rng: 600 if fr % 10 == 3 else int(rng.integers(16, 131)))


def per_frame_values(p, M, k, d_init, frames):
    """Every frame of `frames` evaluated ALONE with its motion estimate (M, k) of the whole range: loss and derivative at
    LOSS_DELAYS and the five-delay batch at BATCH_DELAYS -> (L [F][2], G [F][2], B [F][5]); rows of other frames are NaN"""
    F = len(k)
    L, G, B = np.full((F, 2), np.nan), np.full((F, 2), np.nan), np.full((F, 5), np.nan)
    for f in frames:
        p.init_motion(d_init, f, f)
        p.set_motion(M[f:f + 1], k[f:f + 1])
        L[f], G[f] = p.loss(LOSS_DELAYS, grad=True)
        B[f] = p.loss(BATCH_DELAYS)
    return L, G, B


def window_values(p, M, k, d_init, begin, length):
    """The same three evaluations on the window as ONE selection, with the same motion estimates -> (L [2], G [2], B [5])"""
    p.init_motion(d_init, begin, begin + length - 1)
    p.set_motion(M[begin:begin + length], k[begin:begin + length])
    L, G = p.loss(LOSS_DELAYS, grad=True)
    return L, G, p.loss(BATCH_DELAYS)


def plan_sums(rows, begin, length):
    """plan_sum of every column of rows[begin : begin + length]"""
    rows = np.asarray(rows)
    return np.array([plan_sum(rows[begin:begin + length, c], begin) for c in range(rows.shape[1])])
