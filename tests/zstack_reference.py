"""The Z-stack operators in plain numpy, sharing nothing with the library (include/amt_hip.h states the definitions).

For a (Z, H, W) uint8 / uint16 stack with planes P_z:
  L_z(y, x) = 4 P(y, x) - P(y-1, x) - P(y+1, x) - P(y, x-1) - P(y, x+1), coordinates clamped to the image;
  E_z(y, x) = the sum of L_z^2 over the (2 r + 1)^2 window around (y, x), positions outside the image counting 0;
  index(y, x) = the smallest z at which E_z(y, x) is largest.
Everything is Python-exact: int64 arrays (E < 2^46) and ``Fraction`` for the scores.  Not collected by pytest."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

COLS = ("sum", "sumsq", "lap_sumsq", "brenner")


def laplacian(plane) -> np.ndarray:
    """L of one plane as int64, by edge padding"""
    p = np.pad(np.asarray(plane).astype(np.int64), 1, mode="edge")
    return 4 * p[1:-1, 1:-1] - p[:-2, 1:-1] - p[2:, 1:-1] - p[1:-1, :-2] - p[1:-1, 2:]


def energy(plane, r: int) -> np.ndarray:
    """E of one plane as int64: window sums of L^2 by zero-padded cumulative sums"""
    sq = laplacian(plane) ** 2
    H, W = sq.shape
    c = np.zeros((H + 2 * r + 1, W + 2 * r + 1), np.int64)
    c[r + 1:r + 1 + H, r + 1:r + 1 + W] = sq
    c = c.cumsum(axis=0).cumsum(axis=1)
    k = 2 * r + 1
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def focus_index(stack, r: int) -> np.ndarray:
    """(H, W) uint16: a strict > update over z keeps the smallest z among equals"""
    stack = np.asarray(stack)
    best = energy(stack[0], r)
    index = np.zeros(stack.shape[1:], np.uint16)
    for z in range(1, stack.shape[0]):
        e = energy(stack[z], r)
        better = e > best
        best[better] = e[better]
        index[better] = z
    return index


def z_take(stack, index) -> np.ndarray:
    stack = np.asarray(stack)
    z = np.minimum(np.asarray(index).astype(np.int64), stack.shape[0] - 1)
    return np.take_along_axis(stack, z[None], axis=0)[0]


def focus_stack(stack, r: int) -> np.ndarray:
    return z_take(stack, focus_index(stack, r))


def focus_sums(stack) -> np.ndarray:
    """(Z, 4) int64 in COLS order (Python integers summed exactly, then stored)"""
    out = np.zeros((len(stack), 4), np.int64)
    for z, plane in enumerate(np.asarray(stack)):
        p = plane.astype(np.int64)
        d = p[:, 2:] - p[:, :-2]
        out[z] = (int(p.sum()), int((p * p).sum()), int((laplacian(plane) ** 2).sum()), int((d * d).sum()))
    return out


def focus_scores(stack, method: str) -> np.ndarray:
    """float64 (Z,): exact rationals rounded once"""
    n = int(np.asarray(stack).shape[1] * np.asarray(stack).shape[2])
    out = []
    for s, ss, lap, br in focus_sums(stack).tolist():
        if method == "laplacian_variance":
            out.append(float(Fraction(lap, n)))
        elif method == "normalized_variance":
            out.append(float(Fraction(n * ss - s * s, n * s)) if s else 0.0)
        elif method == "brenner":
            out.append(float(Fraction(br)))
        else:
            raise ValueError(method)
    return np.array(out, dtype=np.float64)


def best_focus_index(stack, method: str = "laplacian_variance") -> int:
    return int(np.argmax(focus_scores(stack, method)))


def z_project(stack, method: str) -> np.ndarray:
    stack = np.asarray(stack)
    if method == "max":
        return stack.max(axis=0)
    if method == "min":
        return stack.min(axis=0)
    if method == "mean":
        if stack.dtype == np.float64:  # the sum in the order z = 0, 1, ..., divided once
            acc = stack[0].copy()
            for z in range(1, len(stack)):
                acc = acc + stack[z]
            return acc / float(len(stack))
        # the exact integer sum divided once
        return stack.astype(np.int64).sum(axis=0).astype(np.float64) / float(len(stack))
    raise ValueError(method)


def median_nearest(index, size: int) -> np.ndarray:
    """The median of a size x size window with edge replication (the ``smooth`` step of extended_depth_of_field)"""
    r = size // 2
    p = np.pad(np.asarray(index), r, mode="edge")
    H, W = np.asarray(index).shape
    win = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(size) for dx in range(size)])
    return np.sort(win, axis=0)[size * size // 2]


def extended_depth_of_field(stack, r: int = 4, smooth: int = 0):
    """(composite, index map)"""
    index = focus_index(stack, r)
    if smooth:
        index = median_nearest(index, smooth)
    return z_take(stack, index), index
