"""tests/lmeds_reference.py pinned to the oracle, without a GPU: guess_winner64 -- the first-wins arg-min of the fp64 lower quartile
over the sampler's row pairs -- is the oracle's GuessMotion (core_private.cpp:34-59 as oracle/rssync_oracle.c restates it) on
ordinary frames and on TILED frames (m distinct tracks x copies), where whole classes of hypotheses have quartiles equal bit for
bit and a pair of copies of one track gives v = 0 exactly: quartile 0, M = 0, and the first such pair wins.  And the census of
the sampler that the tie cases of tests/test_gpu_guess_motion.py rest on."""
import numpy as np
import pytest

from oracle import oracle as ora
from oracle.oracle import OracleProblem, sample_pair
from rssync_amd import synth

import lmeds_reference as ref

SEED, D0, F = 4242, 0.03, 6
STREAM = ora.STREAM_SYNC_INIT + 0


def _oracle(frames, gyro):
    o = OracleProblem(seed=SEED, faithful=False)
    o.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    for fr in frames:
        o.SetTrackResult(*fr)
    return o


def _scene(n, scene_seed, copies=1, **kw):
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, seed=scene_seed)
    frames = [(fr, np.tile(ta, copies), np.tile(tb, copies), np.tile(ra, (copies, 1)), np.tile(rb, (copies, 1)))
              for fr, ta, tb, ra, rb in synth.make_frames(gyro, 0, F, n, seed=scene_seed, **kw)]
    return gyro, frames


def test_ordinary_frames():
    gyro, frames = _scene(600, 31, noise=1e-3)
    o = _oracle(frames, gyro)
    for f in range(F):
        P = o.problem_matrix(f, D0)
        pairs = [sample_pair(SEED, f, STREAM, h, len(P)) for h in range(200)]
        M, bh, med = o.guess_motion(f, D0, 200, STREAM)
        assert ref.guess_winner64(P, pairs) == bh
        assert med > 0.0 and ref.lower_quartile_fp64(P, *pairs[bh]) == pytest.approx(med, rel=1e-9)


@pytest.mark.parametrize("m,copies", [(16, 128), (8, 256), (32, 64), (64, 32)])
def test_tiled_frames_exact_ties(m, copies):
    gyro, frames = _scene(m, 83, copies=copies)
    o = _oracle(frames, gyro)
    for f in range(F):
        P = o.problem_matrix(f, D0)
        assert len(P) == m * copies
        pairs = [sample_pair(SEED, f, STREAM, h, len(P)) for h in range(200)]
        M, bh, med = o.guess_motion(f, D0, 200, STREAM)
        assert ref.guess_winner64(P, pairs) == bh
        # the winner is the FIRST pair of copies of one track: v = P x P = 0 exactly, every residual 0
        same = [h for h, (i0, i1) in enumerate(pairs) if i0 % m == i1 % m]
        assert same and bh == same[0] and med == 0.0 and not M.any()


def test_sampler_census_of_the_three_track_tiling():
    """3 tracks x 682 copies (tests/test_gpu_guess_motion.py: the record table's overflow): of the 200 hypotheses of each of the
    frames 0 .. 5, every class {i0 mod 3, i1 mod 3} of two DIFFERENT tracks -- one direction, one quartile, bit for bit -- has at
    least 25 members (measured: 34 .. 54), one more than the 24 records of the tile kernel's table"""
    n = 3 * 682
    for f in range(F):
        cls = {}
        for h in range(200):
            i0, i1 = sample_pair(SEED, f, STREAM, h, n)
            if i0 % 3 != i1 % 3:
                key = frozenset((i0 % 3, i1 % 3))
                cls[key] = cls.get(key, 0) + 1
        assert len(cls) == 3 and min(cls.values()) >= 25, (f, cls)
