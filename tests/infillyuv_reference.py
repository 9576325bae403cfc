"""numpy restatement of the infill for 4:2:2 and 4:4:4 video (include/rssync_infillyuv.h): a plane is a camera, so a plane's
placement IS the gray infill's (tests/infill_reference.py: first_hits, compose) with that plane's camera -- for a 4:2:2 chroma
plane tests/yuv_reference.py's chroma lens and chroma output camera, the frame times themselves and the plane rows x cols / 2,
against the frames' one target each.  The luma plane, and every plane of a 4:4:4 frame, has infill_reference's placement.

  video         the quality scene in 4:2:2: infill_reference.video()'s seven luma frames, and U and V rendered as
                yuv_reference.scene() renders its three
  chroma_hits   infill_reference.first_hits of the 4:2:2 chroma plane
  figures       per chroma plane (U, V) and frame 32, 33, 34: the samples outside the frame's own plane, how many of them a
                neighbour sees, the error of the borrowed samples and of the constant fill against the global-shutter truth,
                and the samples a position within the device tolerance of an edge could place elsewhere
  counts        the first two of those alone: a siting's placement without its pictures
  error_margin  what the device's error figure may differ by from the restatement's, from that tolerance alone

The scene is rectify_reference.scene()'s gyro and lens at 380 x 676, the delay synth.D_TRUE.
"""
import functools

import numpy as np

import color_reference as cr
import infill_reference as ir
import rectify_reference as rr
import stabilize_reference as sr
import yuv_reference as yr
from rssync_amd import synth, synth_video as sv

RADIUS = ir.RADIUS
CENTER, LEFT = yr.CENTER, yr.LEFT

# Frames 30 .. 36 of the scene's video, targets ir.video_targets(), radius 3, LENS, same size, zoom 1, bilinear, float64 maps;
# the 4:2:2 chroma plane (380 x 338), per frame 32, 33, 34 (the luma rows are infill_reference's: the same camera):
#   OUTSIDE         per siting: samples outside the frame's own plane (U and V: one position)
#   SEEN            ... of which a candidate within the radius sees
#   BORROWED_ERROR  CENTER, per plane U, V: mean absolute grey difference to the truth (yr.truth()) over the borrowed samples
#   FILL_ERROR      ... of the constant fill in the same places: the formats' default, 128
#   NEAR_EDGE       CENTER: samples for which a candidate that was asked lies within yr.device_tolerance(LENS) of an edge of
#                   the plane
#   python -c "import sys; sys.path[:0] = ['.', 'tests']; import infillyuv_reference as iyr; iyr.print_figures()"
OUTSIDE = {CENTER: (4614, 5193, 4699), LEFT: (4610, 5189, 4695)}
SEEN = {CENTER: (4608, 5193, 4695), LEFT: (4604, 5189, 4691)}
BORROWED_ERROR = ((7.788, 11.601, 8.807), (8.899, 13.321, 9.617))
FILL_ERROR = ((35.3, 37.6, 38.0), (37.7, 37.5, 37.7))
NEAR_EDGE = (2, 1, 1)
FILL = 128
# the share of the plane's outside samples that some candidate within radius 3 sees, SEEN / OUTSIDE above, is 0.9987, 1, 0.9991
# at both sitings; rounded down to two places, as infill_reference.MIN_BORROWED_SHARE is
MIN_BORROWED_SHARE = 0.99
# "far below the constant fill's error": at most half of it, as colorinfill_reference has it for the 4:2:0 chroma planes
FAR_BELOW = 0.5


def error_margin(k):
    """Grey levels the device's mean error over its borrowed chroma samples of frame 32 + k may lie from
    BORROWED_ERROR[plane][k], from the device tolerance alone: colorinfill_reference.error_margin's two terms.  (a) A position
    within tol px of the restatement's moves a bilinear value by at most 255 * tol per axis: 2 * 255 * tol; rounding a value
    moved by that much to a byte changes the byte by one level in at most that share of the samples: as much again.  (b) A
    sample with a candidate within tol of an edge may take another donor, or none, and then differ by anything: 255 each,
    over the borrowed samples."""
    return 4.0 * 255.0 * yr.device_tolerance(sr.LENS) + 255.0 * NEAR_EDGE[k] / max(SEEN[CENTER][k], 1)


@functools.lru_cache(maxsize=None)
def video(site=CENTER):
    """-> (Y (7, 380, 676), U, V (7, 380, 338), times (7,)) of frames 30 .. 36 (read-only): Y and the times are
    infill_reference.video()'s; U and V as yuv_reference.scene() renders them, and equal to its planes for frames 32 .. 34"""
    s = yr.scene(site)
    y, times = ir.video()
    planes = []
    for name, seed in (("u", cr.U_SEED), ("v", cr.V_SEED)):
        a, _ = sv.render(s["gyro"], ir.VIDEO[0], ir.VIDEO[1], lens=s["lens_c"], rows=yr.C_ROWS, cols=yr.C_COLS, seed=rr.SEED,
                         d_true=synth.D_TRUE, texture_seed=seed)
        assert (a[ir.VIDEO_SCENE] == s[name]).all()
        a.setflags(write=False)
        planes.append(a)
    return y, planes[0], planes[1], times


def chroma_camera(site=CENTER):
    """-> (lens, rows, cols, frame times, output camera) of the scene's 4:2:2 chroma plane: the times are the frames'"""
    lens = rr.scene()["lens"]
    _, times = ir.video()
    return yr.chroma_lens422(lens, site), yr.C_ROWS, yr.C_COLS, times, yr.chroma_camera422(lens, rr.ROWS, rr.COLS, rr.ROWS, rr.COLS, site)


def chroma_hits(f, radius=RADIUS, site=CENTER):
    """infill_reference.first_hits of frame f of the video in the chroma plane's camera, against the frames' targets"""
    lens, rows, cols, times, cam = chroma_camera(site)
    return ir.first_hits(rr.scene()["gyro"], lens, rows, cols, times, synth.D_TRUE, ir.video_targets(), radius, f, cam=cam)


def near_edge_count(f, place, radius=RADIUS, site=CENTER):
    """samples of frame f for which a candidate that was asked -- the donor and every candidate before it, or all of them
    where none hit -- lies within the device tolerance of an edge of the plane"""
    lens, rows, cols, times, cam = chroma_camera(site)
    tol = yr.device_tolerance(sr.LENS)
    near = np.zeros(place.shape, bool)
    for k, g in enumerate(ir.candidates(f, len(times), radius)):
        m = sr.map64(rr.scene()["gyro"], lens, rows, cols, times[g], synth.D_TRUE, target=ir.video_targets()[f], cam=cam)
        near |= sr.near_edge(m, rows, cols, tol) & ((place < 0) | (place >= k))
    return int(near.sum())


def _scene_frames():
    _, times = ir.video()
    return list(enumerate(range(*ir.VIDEO_SCENE.indices(len(times)))))


def counts(site):
    """per frame 32, 33, 34 -> (outside, seen) of the chroma plane at a siting"""
    out = []
    for _, f in _scene_frames():
        place, _, _ = chroma_hits(f, site=site)
        out.append((int((place != 0).sum()), int((place > 0).sum())))
    return out


def figures():
    """CENTER siting; per chroma plane (0: U, 1: V) and frame 32, 33, 34 -> (outside, seen, borrowed error, fill error, near
    edge)"""
    _, u, v, times = video()
    truth = yr.truth(CENTER)
    hits = {f: chroma_hits(f) for _, f in _scene_frames()}
    near = {f: near_edge_count(f, hits[f][0]) for f in hits}
    out = {}
    for p, frames in enumerate((u, v)):
        rows = []
        for k, f in _scene_frames():
            place, pos, _ = hits[f]
            img = ir.compose(frames, place, pos, ir.candidates(f, len(times), RADIUS), fill=FILL)
            lent = place > 0
            tr = truth[p][k].astype(np.float64)
            diff = np.abs(img.astype(np.float64) - tr)
            rows.append((int((place != 0).sum()), int(lent.sum()), float(diff[lent].mean()), float(np.abs(FILL - tr)[lent].mean()), near[f]))
        out[p] = rows
    return out


def print_figures():
    fig = figures()
    for site, name in ((CENTER, "CENTER"), (LEFT, "LEFT")):
        c = [(r[0], r[1]) for r in fig[0]] if site == CENTER else counts(site)
        print("%s outside %s seen %s shares %s" % (name, tuple(o for o, _ in c), tuple(s for _, s in c), [round(s / o, 5) for o, s in c]))
    for name, col, fmt in (("BORROWED_ERROR", 2, "%.3f"), ("FILL_ERROR", 3, "%.1f")):
        print("%s = (%s)" % (name, ", ".join("(" + ", ".join(fmt % r[col] for r in fig[p]) + ")" for p in (0, 1))))
    print("NEAR_EDGE = (%s)" % ", ".join("%d" % r[4] for r in fig[0]))
