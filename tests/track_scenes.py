"""Synthetic frame pairs for the tracker tests: band-limited texture evaluated exactly at any position, so that a pair
shifted by a known (sub-pixel or large) amount has a known ground truth."""
import numpy as np


def texture(x, y, lo, hi, seed=5):
    """band-limited pattern evaluated exactly at any position: 16 sinusoids, wavelengths lo .. hi px, every direction"""
    rng = np.random.default_rng(seed)
    v = np.zeros(np.broadcast(x, y).shape)
    for _ in range(16):
        lam, th, ph = rng.uniform(lo, hi), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        v += np.sin(2 * np.pi / lam * (np.cos(th) * x + np.sin(th) * y) + ph)
    return np.clip(np.rint(128 + 30 * v), 0, 255).astype(np.uint8)


def shifted_pair(sx, sy, lo, hi, w=420, h=340):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([texture(xs, ys, lo, hi), texture(xs - sx, ys - sy, lo, hi)])   # content moves by (+sx, +sy)


def multiscale(x, y, lo=8.0, hi=512.0, seed=9):
    """texture at every pyramid level: 24 sinusoids with wavelengths spread log-uniformly over lo .. hi px, so that a
    level l of scale 2^l still sees the ones longer than ~4 * 2^l px"""
    rng = np.random.default_rng(seed)
    v = np.zeros(np.broadcast(x, y).shape)
    for lam in np.exp(rng.uniform(np.log(lo), np.log(hi), 24)):
        th, ph = rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        v += np.sin(2 * np.pi / lam * (np.cos(th) * x + np.sin(th) * y) + ph)
    return np.clip(np.rint(128 + 22 * v), 0, 255).astype(np.uint8)


def multiscale_frames(w, h, shifts, seed=9):
    """(n, h, w) uint8: frame k is the multiscale texture moved by shifts[k] = (sx, sy)"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([multiscale(xs - sx, ys - sy, seed=seed) for sx, sy in shifts])
