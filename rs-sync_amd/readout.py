"""Estimating the sensor's rolling-shutter readout time from the data (SyncProblem.readout_sweep).

A ray's time is frame_time + ro * y / rows (core_testcode.cpp:144-145).  The library takes ``ro`` from the caller; a
wrong one does not make the solver fail, it moves the delay by about half the error.  PreSync's cost has a shallow,
convex minimum over ``ro``: sweep a grid of readouts, take the arg-min (PreSync's own rule, lexicographic on
(cost, delay)), and install it with ``set_readout`` before Sync.
"""
from collections import namedtuple

import numpy as np

ReadoutEstimate = namedtuple("ReadoutEstimate", "readout delay cost vertex vertex_is_interior readouts costs delays")
ReadoutEstimate.__doc__ = """\
readout, delay, cost: the grid point with the lowest (cost, delay) and its PreSync result;
vertex: the vertex of the parabola through the arg-min and its two neighbours (the grid point itself where the arg-min
lies on the edge of the grid or the three points do not open upwards), vertex_is_interior: whether it is such a vertex;
readouts, costs, delays: the whole sweep."""


def grid_vertex(x, costs, k):
    """The refinement rule of the grid searches (estimate_readout here, rssync_amd.lens.estimate_lens): the vertex of
    the parabola through the arg-min k of an ascending grid x and its two neighbours, clamped to them -> (vertex,
    interior).  Where k lies on the grid's edge or the three points do not open upwards: (x[k], False)."""
    vertex, interior = float(x[k]), False
    if 0 < k < len(x) - 1:
        x0, x1, x2 = x[k - 1:k + 2]
        y0, y1, y2 = costs[k - 1:k + 2]
        # the parabola through the three points, in divided differences
        d01, d12 = (y1 - y0) / (x1 - x0), (y2 - y1) / (x2 - x1)
        curv = (d12 - d01) / (x2 - x0)
        if curv > 0:
            vertex = float(0.5 * (x0 + x1) - d01 / (2.0 * curv))
            vertex = min(max(vertex, float(x0)), float(x2))
            interior = True
    return vertex, interior


def estimate_readout(problem, readouts, initial_delay, frame_begin, frame_end, search_step, search_radius):
    """Sweep the candidate readouts (s, ascending) over the pixel frames of [frame_begin, frame_end) -> ReadoutEstimate.
    The frames keep their own readout; install the estimate with problem.set_readout(est.readout)."""
    ro = np.ascontiguousarray(readouts, np.float64).reshape(-1)
    if ro.size > 1 and not np.all(np.diff(ro) > 0):
        raise ValueError("readouts must be ascending")
    costs, delays = problem.readout_sweep(ro, initial_delay, frame_begin, frame_end, search_step, search_radius)
    k = min(range(ro.size), key=lambda i: (costs[i], delays[i]))
    vertex, interior = grid_vertex(ro, costs, k)
    return ReadoutEstimate(float(ro[k]), float(delays[k]), float(costs[k]), vertex, interior, ro, costs, delays)
