"""Applying a camera order (``Solver.covisibility``'s ``order``) to a window by hand.

``Solver.solve(prob, order=...)`` does this inside the library; ``permute_cams`` / ``restore_cams`` give the same
to the calls that take a window as it is (``covariance``, ``residuals``, ``lm_step``, ``prepare``): permute, call,
and map camera-indexed results back with ``order`` (position k of the permuted window is camera ``order[k]``).
"""
from __future__ import annotations

import numpy as np

from .capi import ProblemArrays


def inverse_order(order) -> np.ndarray:
    """inv[c] = the position of camera c; raises unless ``order`` is a permutation."""
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    if not np.array_equal(np.sort(order), np.arange(len(order))):
        raise ValueError("order is not a permutation of 0 .. n_cams-1")
    inv = np.empty(len(order), dtype=np.int64)
    inv[order] = np.arange(len(order))
    return inv


def permute_cams(prob: ProblemArrays, order) -> ProblemArrays:
    """The window with camera ``order[k]`` placed k-th: cameras permuted, ``obs_cam`` and ``fixed_cam`` remapped.
    Cameras and ``obs_cam`` are new arrays; points, intrinsics and the other observation arrays are SHARED with
    ``prob`` (a solve of the result updates ``prob``'s points and intrinsics, as ba_solve_ordered does)."""
    inv = inverse_order(order)
    if len(inv) != prob.n_cams:
        raise ValueError("order must have one entry per camera")
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    fixed = int(inv[prob.fixed_cam]) if 0 <= prob.fixed_cam < prob.n_cams else int(prob.fixed_cam)
    return ProblemArrays(prob.cams[order], prob.points, prob.intr, prob.intr_prior, inv[prob.obs_cam].astype(np.int32),
                         prob.obs_pt, prob.obs_uv, prob.obs_depth, fixed, dict(prob.meta))


def restore_cams(prob: ProblemArrays, permuted: ProblemArrays, order) -> None:
    """Copy the cameras of ``permuted`` (= permute_cams(prob, order), after a solve) back to ``prob``'s numbering."""
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    prob.cams[order] = permuted.cams
