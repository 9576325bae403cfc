"""numpy restatement of the colour infill (include/rssync_colorinfill.h): a plane is a camera, so a plane's placement IS
the gray infill's (tests/infill_reference.py: first_hits, compose) with that plane's camera -- for a 4:2:0 chroma plane
tests/color_reference.py's chroma lens, chroma frame times and chroma output camera, against the frames' one target each.

  video         the quality scene in colour: infill_reference.video()'s seven luma frames, and U and V rendered as
                color_reference.scene() renders its three
  chroma_hits   infill_reference.first_hits of a chroma plane
  figures       per plane (Y, U, V) and frame 32, 33, 34: the samples outside the frame's own plane, how many of them a
                neighbour sees, the error of the borrowed samples and of the constant fill against the global-shutter truth,
                and the samples a position within the device tolerance of an edge could place elsewhere
  error_margin  what the device's error figure may differ by from the restatement's, from that tolerance alone

The scene is rectify_reference.scene()'s gyro and lens at 380 x 676, the delay synth.D_TRUE, the chroma site CENTER.
"""
import functools

import numpy as np

import color_reference as cr
import infill_reference as ir
import rectify_reference as rr
import stabilize_reference as sr
from rssync_amd import synth, synth_video as sv

RADIUS = ir.RADIUS
SITE = cr.CENTER

# Frames 30 .. 36 of the scene's video, targets ir.video_targets(), radius 3, LENS, same size, zoom 1, bilinear, float64 maps;
# per plane Y, U, V and per frame 32, 33, 34 (plane Y's first four rows are infill_reference's figures: the same camera):
#   OUTSIDE         samples outside the frame's own plane
#   SEEN            ... of which a candidate within the radius sees
#   BORROWED_ERROR  mean absolute grey difference to the truth (sr.truth(), cr.truth()) over the borrowed samples
#   FILL_ERROR      ... of the constant fill in the same places: the formats' default, FILL
#   NEAR_EDGE       samples for which a candidate that was asked lies within cr.device_tolerance(LENS) (chroma) or
#                   sr.device_tolerance(LENS) (luma) of an edge of its plane
#   python -c "import sys; sys.path[:0] = ['.', 'tests']; import colorinfill_reference as cir; cir.print_figures()"
OUTSIDE = ((9033, 10314, 9215), (2414, 2675, 2432), (2414, 2675, 2432))
SEEN = ((9022, 10314, 9208), (2409, 2675, 2428), (2409, 2675, 2428))
BORROWED_ERROR = ((8.865, 12.924, 9.715), (7.780, 11.658, 8.877), (8.902, 13.419, 9.676))
FILL_ERROR = ((122.1, 116.8, 115.6), (35.3, 37.5, 37.9), (37.7, 37.7, 37.7))
NEAR_EDGE = ((3, 1, 2), (0, 0, 1), (0, 0, 1))
FILL = (0, 128, 128)
# the share of a plane's outside samples that some candidate within radius 3 sees, SEEN / OUTSIDE above, is 0.99878, 1, 0.99924
# (Y) and 0.99793, 1, 0.99836 (U, V); rounded down to two places, as infill_reference.MIN_BORROWED_SHARE is
MIN_BORROWED_SHARE = (0.99, 0.99, 0.99)
# "far below the constant fill's error": at most half of it.  Mid-grey is the best constant a chroma plane can get -- the
# restatement's borrowed samples are at 0.21 to 0.36 of it there, and at 0.07 to 0.11 of black in the luma plane
FAR_BELOW = 0.5


def error_margin(plane, k):
    """Grey levels the device's mean error over its borrowed samples may lie from BORROWED_ERROR[plane][k], from the device
    tolerance alone.  (a) A position within tol px of the restatement's moves a bilinear value by at most 255 * tol per axis:
    2 * 255 * tol; rounding a value moved by that much to a byte changes the byte by one level in at most that share of the
    samples: as much again.  (b) A sample with a candidate within tol of an edge may take another donor, or none, and then
    differ by anything: 255 each, over the borrowed samples."""
    tol = sr.device_tolerance(sr.LENS) if plane == 0 else cr.device_tolerance(sr.LENS)
    return 4.0 * 255.0 * tol + 255.0 * NEAR_EDGE[plane][k] / max(SEEN[plane][k], 1)


@functools.lru_cache(maxsize=None)
def video():
    """-> (Y (7, 380, 676), U, V (7, 190, 338), times (7,)) of frames 30 .. 36 (read-only): Y and the times are
    infill_reference.video()'s; U and V as color_reference.scene() renders them, and equal to its planes for frames 32 .. 34"""
    s = cr.scene(SITE)
    y, times = ir.video()
    d = synth.D_TRUE + s["lens"][0] * cr.OFFSET[SITE][1] / rr.ROWS
    planes = []
    for name, seed in (("u", cr.U_SEED), ("v", cr.V_SEED)):
        a, _ = sv.render(s["gyro"], ir.VIDEO[0], ir.VIDEO[1], lens=s["lens_c"], rows=cr.C_ROWS, cols=cr.C_COLS, seed=rr.SEED, d_true=d,
                         texture_seed=seed)
        assert (a[ir.VIDEO_SCENE] == s[name]).all()
        a.setflags(write=False)
        planes.append(a)
    return y, planes[0], planes[1], times


def plane_camera(plane):
    """-> (lens, rows, cols, frame times, output camera or None) of plane 0 (Y) or of a chroma plane (1, 2) of the scene"""
    s = rr.scene()
    _, times = ir.video()
    if plane == 0:
        return s["lens"], rr.ROWS, rr.COLS, times, None
    lens = s["lens"]
    times_c = np.array([cr.chroma_time(t, lens, rr.ROWS, SITE) for t in times])
    return cr.chroma_lens(lens, SITE), cr.C_ROWS, cr.C_COLS, times_c, cr.chroma_camera(lens, rr.ROWS, rr.COLS, rr.ROWS, rr.COLS, SITE)


def plane_hits(plane, f, radius=RADIUS):
    """infill_reference.first_hits of frame f of the video in a plane's camera, against the frames' targets"""
    s = rr.scene()
    lens, rows, cols, times, cam = plane_camera(plane)
    return ir.first_hits(s["gyro"], lens, rows, cols, times, synth.D_TRUE, ir.video_targets(), radius, f, cam=cam)


def chroma_hits(f, radius=RADIUS):
    return plane_hits(1, f, radius)


def near_edge_count(plane, f, place, radius=RADIUS):
    """samples of frame f for which a candidate that was asked -- the donor and every candidate before it, or all of them
    where none hit -- lies within the device tolerance of an edge of the plane"""
    s = rr.scene()
    lens, rows, cols, times, cam = plane_camera(plane)
    tol = sr.device_tolerance(sr.LENS) if plane == 0 else cr.device_tolerance(sr.LENS)
    near = np.zeros(place.shape, bool)
    for k, g in enumerate(ir.candidates(f, len(times), radius)):
        m = sr.map64(s["gyro"], lens, rows, cols, times[g], synth.D_TRUE, target=ir.video_targets()[f], cam=cam)
        near |= sr.near_edge(m, rows, cols, tol) & ((place < 0) | (place >= k))
    return int(near.sum())


def figures(planes=(0, 1, 2)):
    """per plane and frame 32, 33, 34 -> (outside, seen, borrowed error, fill error, near edge)"""
    y, u, v, times = video()
    frames, truth = (y, u, v), (sr.truth(),) + tuple(cr.truth(SITE))
    out = {}
    for plane in planes:
        rows = []
        for k, f in enumerate(range(*ir.VIDEO_SCENE.indices(len(times)))):
            place, pos, _ = plane_hits(min(plane, 1), f)
            img = ir.compose(frames[plane], place, pos, ir.candidates(f, len(times), RADIUS))
            lent = place > 0
            tr = truth[plane][k].astype(np.float64)
            diff = np.abs(img.astype(np.float64) - tr)
            rows.append((int((place != 0).sum()), int(lent.sum()), float(diff[lent].mean()), float(np.abs(FILL[plane] - tr)[lent].mean()),
                         near_edge_count(min(plane, 1), f, place)))
        out[plane] = rows
    return out


def print_figures():
    fig = figures()
    for name, col, fmt in (("OUTSIDE", 0, "%d"), ("SEEN", 1, "%d"), ("BORROWED_ERROR", 2, "%.3f"), ("FILL_ERROR", 3, "%.1f"), ("NEAR_EDGE", 4, "%d")):
        print("%s = (%s)" % (name, ", ".join("(" + ", ".join(fmt % r[col] for r in fig[p]) + ")" for p in (0, 1, 2))))
    print("shares", [[round(r[1] / r[0], 5) for r in fig[p]] for p in (0, 1, 2)])
