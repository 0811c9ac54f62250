"""csrc/ordered_sum.h restated in NumPy for the test doubles of the ensemble metrics: every sum sequential from +0.0 in index order
(numpy.sum adds pairwise), every result written through the policy the caller names.  tests/test_ordered_sum_cpu.py holds these
functions to the header, compiled for the host, bit for bit."""
import numpy as np

THREADS, GROUP = 256, 16
GROUPS = THREADS // GROUP


def nan_if_nan(t):
    """the canonical NaN for a NaN; an infinite sum stays"""
    return np.where(np.isnan(t), np.nan, t)


def nan_if_not_finite(t):
    """the canonical NaN for a NaN and for +-inf"""
    return np.where(np.isfinite(t), t, np.nan)


def seq_sum(a, axis):
    """the sum along `axis` in index order from +0.0, one addition after the other"""
    a = np.moveaxis(np.asarray(a, np.float64), axis, 0)
    t = np.zeros(a.shape[1:], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(a.shape[0]):
            t = t + a[k]
    return t


def fold_workgroup(acc, policy):
    """acc (..., N, 256) float64, the accumulators of a workgroup's threads -> (..., N): sixteen threads at a time in thread order,
    then the sixteen group totals in group order (stash, fold_groups, fold_total), written through `policy`"""
    acc = np.asarray(acc, np.float64)
    assert acc.shape[-1] == THREADS
    groups = acc.reshape(acc.shape[:-1] + (GROUPS, GROUP))
    return policy(seq_sum(seq_sum(groups, -1), -1))


def fold_parts(part, axis, policy):
    """the sum over the chunks or tiles along `axis`, in index order (fold_parts), written through `policy`"""
    return policy(seq_sum(part, axis))
