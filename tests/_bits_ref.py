"""
Float64 numpy reference of k_fwd_gt_bits (skdist_amd/ops/csrc/
sgd_kernels.hip), the twin of ``_dense_ref.ref_gt`` for per-element targets
and train masks, and the packer from 0/1 matrices to the int32 bit planes
the kernel reads.  Matrices are in shuffled row order (the order of ``Xs``).

A plain helper module, not a conftest.
"""

import numpy as np

import _dense_ref as R


def pack_plane(a, n_pad, ncols_pad):
    """0/1 matrix [n, ncols] -> int32 [n_pad, ncols_pad // 32]: bit
    ``c & 31`` of word ``[r, c >> 5]`` is ``a[r, c]``; rows >= n and columns
    >= ncols are 0."""
    a = np.asarray(a)
    n, ncols = a.shape
    assert ncols_pad % 32 == 0 and n <= n_pad and ncols <= ncols_pad
    full = np.zeros((n_pad, ncols_pad), np.uint64)
    full[:n, :ncols] = a != 0
    shifts = np.arange(32, dtype=np.uint64)
    words = (full.reshape(n_pad, ncols_pad // 32, 32) << shifts).sum(
        axis=2, dtype=np.uint64)
    return words.astype(np.uint32).view(np.int32)


def unpack_plane(words, ncols_pad):
    """Inverse of ``pack_plane``: int32 words -> 0/1 [n_pad, ncols_pad]."""
    w = np.ascontiguousarray(words).view(np.uint32).astype(np.uint64)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(w.shape[0], ncols_pad).astype(np.uint8)


def ref_gt_bits(Xs, WbfT, fold, col_fold, row_w, targets, mask, start, m,
                loss_id):
    """K1 (k_fwd_gt_bits).  Xs [n_pad, fa], WbfT [ncols_pad, fa], fold [n],
    col_fold [ncols_pad], row_w [n] or None, targets / mask [n, ncols] of
    0/1 (mask None: every element may train).

    Returns (z, g, train), each [m_pad, ncols_pad], with ``_dense_ref``'s
    padding rules: z = Xs[start:start+m_pad]·WbfTᵀ, g = dloss(z, target) *
    row_w where the element trains, else 0.  An element trains when the row
    is below m, the row's fold differs from the column's and its mask bit
    is set.  Rows at or past n read fold = -9, row_w = 1, target = 0 and
    mask = 0 (all ones without a mask); pad columns read target = mask = 0.
    """
    Xs = np.asarray(Xs, np.float64)
    WbfT = np.asarray(WbfT, np.float64)
    n = len(fold)
    ncp = WbfT.shape[0]
    m_pad = R.ceil_to(m, 128)
    rows = start + np.arange(m_pad)
    ok = rows < n
    rc = np.minimum(rows, n - 1)
    fv = np.where(ok, np.asarray(fold)[rc], -9)
    rw = np.ones(m_pad)
    if row_w is not None:
        rw = np.where(ok, np.asarray(row_w, np.float64)[rc], 1.0)
    cfo = np.asarray(col_fold).astype(np.int64)

    def plane(a):
        a = np.asarray(a)
        full = np.zeros((m_pad, ncp))
        full[:, : a.shape[1]] = np.where(ok[:, None], a[rc] != 0, 0)
        return full

    t = plane(targets)
    z = Xs[start:start + m_pad] @ WbfT.T
    g = R.dloss(loss_id, z, t) * rw[:, None]
    train = (fv[:, None] != cfo[None, :]) & (np.arange(m_pad) < m)[:, None]
    if mask is not None:
        train = train & (plane(mask) != 0)
    return z, np.where(train, g, 0.0), train
