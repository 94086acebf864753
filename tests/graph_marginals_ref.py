"""Host reference for slam_graph_marginals: selected columns of H^-1.

``ref_columns`` refines NumPy's float64 inverse with residuals formed in
extended precision, so the reference's own error (``spread``) is known and the
GPU tests' bars are set from it, not from what the device returns.
``gate`` is the reference's test before it inverts H (graph_based_slam.py:496).
"""
import numpy as np


def ref_columns(H, cols):
    """(X64, Xref, spread): X64 = inv(H)[:, cols]; Xref = X64 refined four times
    by X += inv(H) (E - H X) with the residual in np.longdouble; spread =
    max|Xref - X64|."""
    H = np.asarray(H, dtype=np.float64)
    cols = np.asarray(cols, dtype=np.int64)
    Hinv = np.linalg.inv(H)
    X64 = Hinv[:, cols].copy()
    E = np.zeros((H.shape[0], len(cols)), dtype=np.longdouble)
    E[cols, np.arange(len(cols))] = 1.0
    Hl = H.astype(np.longdouble)
    X = X64.astype(np.longdouble)
    for _ in range(4):
        R = E - Hl @ X
        X = X + (Hinv @ R.astype(np.float64)).astype(np.longdouble)
    Xref = X.astype(np.float64)
    return X64, Xref, float(np.abs(Xref - X64).max())


def gate(H, det_min=0.1, cond_max=1e15):
    """updateEstPose's gate (:494-496): det_min < det(H) and cond(H) < cond_max."""
    return bool(det_min < np.linalg.det(H) and np.linalg.cond(H) < cond_max)


def unknowns(all_times, times):
    """Indices of the 3 unknowns of each of ``times`` in the system over the
    sorted ``all_times``."""
    pos = {int(t): k for k, t in enumerate(all_times)}
    return np.array([3 * pos[int(t)] + q for t in times for q in range(3)], dtype=np.int64)
