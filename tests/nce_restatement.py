"""A restatement of the negative rows of the NCE region loss (`csrc/nce_index.h`, visual_target == 2) in numpy, built on the
hash of tests/dropout_restatement.py. Test infrastructure: tests/test_nce_index.py pins it bit for bit against the header
itself (compiled for the host, tests/nce_index_driver.cpp); tests/test_nce_loss_gpu.py then holds the index kernel to it and
restates the negatives of a model step from `model._nce_seed`.

    R = regions WITHOUT the global row, g = b * R + r the labelled region, n_neg = n_across + n_inside
    h(k) = vb_hash(s, (g * n_neg + j) * 2 + k)        s = the launch seed (after the device step counter, seed_with_epoch)
    scale(x, m) = (uint64(x) * m) >> 32
    j <  n_across:  rb = scale(h(0), B - 1), rb == b -> B - 1;  rc = scale(h(1), R);                  row rb * R + rc
    j >= n_across:  rc = scale(h(1), R - 1), rc == r -> R - 1;                                        row b * R + rc
"""
import numpy as np

import dropout_restatement as DR


def _scale(x, m):
    return ((x.astype(np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def negatives(seed, region_idx, batch, regions, n_across, n_inside, epoch=None):
    """int64 [rows, n_across + n_inside]: the table rows of the negatives of the labelled regions `region_idx` (any integer
    sequence) under host seed `seed`; epoch: the value of a registered device step counter, None = none registered."""
    s = DR.seed_with_epoch(seed, epoch) if epoch is not None else int(seed) & DR.MASK64
    g = np.asarray(region_idx, dtype=np.int64).reshape(-1, 1)
    n_neg = n_across + n_inside
    j = np.arange(n_neg, dtype=np.int64).reshape(1, -1)
    b, r = g // regions, g % regions
    with np.errstate(over="ignore"):
        at = (g.astype(np.uint64) * np.uint64(n_neg) + j.astype(np.uint64)) * np.uint64(2)
        h0, h1 = DR.vb_hash(s, at), DR.vb_hash(s, at + np.uint64(1))
    out = np.empty((g.shape[0], n_neg), dtype=np.int64)
    if n_across > 0:
        rb = _scale(h0[:, :n_across], batch - 1)
        rb = np.where(rb == b, batch - 1, rb)
        out[:, :n_across] = rb * regions + _scale(h1[:, :n_across], regions)
    if n_inside > 0:
        rc = _scale(h1[:, n_across:], regions - 1)
        rc = np.where(rc == r, regions - 1, rc)
        out[:, n_across:] = b * regions + rc
    return out
