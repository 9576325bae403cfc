"""Estimating the lens from the data (SyncProblem.lens_sweep), for a clip that comes without a calibration profile.

PreSync's cost has a minimum over the focal length and over the distortion terms, and a shallow one over the principal
point, while the delay of its arg-min barely moves (one grid step either side).  ``estimate_lens`` walks down that cost one
parameter at a time: a grid of candidates around the current lens, one ``lens_sweep`` call for the whole grid, a move to
the vertex of the parabola through the arg-min and its two neighbours (the rule of rssync_amd.readout), then the next
parameter; after a pass over all parameters the grids shrink.  Nothing is installed: ``problem.set_lens(est.lens)`` does
that, before Sync.

What the data cannot tell, the search cannot find: a camera that only rolls about its optical axis says nothing about
the focal length.  Such a parameter ends with its arg-min on the edge of its last grid and is listed in ``unresolved``.
"""
from collections import namedtuple

import numpy as np

from .readout import grid_vertex

# position in the lens (ro, fx, fy, cx, cy, k1, k2, k3, k4) of the additive parameters
_ADDITIVE = {"ro": 0, "cx": 3, "cy": 4, "k1": 5, "k2": 6}
PARAMS = ("f",) + tuple(_ADDITIVE)
# first-pass half-widths: "f" relative (fx and fy scaled together), the others in their own units (px, s)
DEFAULT_SPANS = {"f": 0.25, "k1": 0.15, "k2": 0.15, "cx": 100.0, "cy": 100.0, "ro": 0.005}

LensPass = namedtuple("LensPass", "param round grid costs delays argmin vertex vertex_is_interior")
LensPass.__doc__ = """\
One sweep of one parameter: grid = the offsets tried around the lens of that moment (relative for "f"), costs / delays =
their PreSync results, argmin = the grid index with the lowest (cost, delay), vertex = the offset the search moved by,
vertex_is_interior = whether that is the vertex of a parabola through three grid points (readout.grid_vertex)."""

LensEstimate = namedtuple("LensEstimate", "lens cost delay passes unresolved")
LensEstimate.__doc__ = """\
lens: the final lens (ro, fx, fy, cx, cy, k1, k2, k3, k4); cost, delay: its PreSync result; passes: every LensPass in
the order it ran; unresolved: the parameters whose arg-min sat on the edge of the grid in the last round -- the data
did not pin them down within the spans given."""


def shifted(lens, param, offset):
    """The lens with one parameter moved: "f" scales fx and fy by (1 + offset), the others add the offset."""
    out = np.array(lens, np.float64)
    if param == "f":
        out[1:3] *= 1.0 + offset
    else:
        out[_ADDITIVE[param]] += offset
    return out


def estimate_lens(problem, lens, initial_delay, frame_begin, frame_end, search_step, search_radius, params=("f", "k1"),
                  spans=None, points=9, rounds=3, shrink=0.4):
    """Coordinate search over `params` from the start `lens`, on the pixel frames of [frame_begin, frame_end) ->
    LensEstimate.  Per round and parameter: np.linspace(-span, span, points) around the current value, one lens_sweep,
    a move to the grid's vertex; the spans (DEFAULT_SPANS, or `spans` by parameter name) shrink by `shrink` per round.
    The grid of "ro" is cut to the current readout where it would reach below zero.  The frames keep their own lens."""
    lens = np.ascontiguousarray(lens, np.float64)
    if lens.shape != (9,):
        raise ValueError("lens = (ro, fx, fy, cx, cy, k1, k2, k3, k4)")
    params = tuple(params)
    for nm in params:
        if nm not in PARAMS:
            raise ValueError("unknown lens parameter %r (one of %s)" % (nm, ", ".join(PARAMS)))
    if points < 3 or rounds < 1 or not 0 < shrink <= 1:
        raise ValueError("points >= 3, rounds >= 1, 0 < shrink <= 1")
    span = dict(DEFAULT_SPANS)
    span.update(spans or {})
    for nm in params:
        if not span[nm] > 0 or (nm == "f" and span[nm] >= 1):
            raise ValueError("span of %r must be positive (and below 1 for \"f\")" % nm)
    args = (initial_delay, frame_begin, frame_end, search_step, search_radius)
    passes = []
    for rnd in range(rounds):
        for nm in params:
            half = span[nm] * shrink ** rnd
            if nm == "ro":
                half = min(half, float(lens[0]))
                if not half > 0:
                    raise ValueError("\"ro\" cannot be searched from a readout of zero")
            grid = np.linspace(-half, half, points)
            costs, delays = problem.lens_sweep(np.stack([shifted(lens, nm, g) for g in grid]), *args)
            k = min(range(points), key=lambda i: (costs[i], delays[i]))
            vertex, interior = grid_vertex(grid, costs, k)
            passes.append(LensPass(nm, rnd, grid, costs, delays, k, vertex, interior))
            lens = shifted(lens, nm, vertex)
    cost, delay = problem.lens_sweep(lens[None, :], *args)
    unresolved = tuple(p.param for p in passes if p.round == rounds - 1 and p.argmin in (0, points - 1))
    return LensEstimate(lens, float(cost[0]), float(delay[0]), passes, unresolved)
