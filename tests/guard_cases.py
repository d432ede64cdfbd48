"""Yardsticks of the skip-non-finite-steps tests (tests/test_host_guard.py, tests/test_gpu_guard.py,
tests/test_gpu_guard_parallel.py) -- not a test module.

The guard's decision: a step is skipped exactly when an element of the trainable ranges of the gradient is NaN or +-Inf
(include/lirec_hip.h, lirec_clip_finalize_guard: the double sum of squares is non-finite exactly then).  The accounting:
torch.optim.Adam keeps one `step` per parameter -- the number of updates IT has received.  `Ledger` counts that by hand, one
call at a time; FusedAdam's (step, lag, S) bookkeeping has to give the same numbers."""
import numpy as np

BAD = {'nan': float('nan'), 'pinf': float('inf'), 'ninf': float('-inf')}
SIZES = [1, 5, 1025]                             # one scalar; one f32x4 and a tail of one; a second block whose tail is one


def positions(n):
    """where the non-finite element goes: in the f32x4 body and in the scalar tail of a range of n elements"""
    return sorted({0, n - 1})


def must_skip(values, ranges):
    """the decision from the values themselves; ranges = [(offset, length), ...]"""
    v = np.asarray(values)
    return any(not np.isfinite(v[o:o + k]).all() for o, k in ranges)


class Ledger:
    """updates received per parameter, counted one optimiser call at a time"""

    def __init__(self, n_params):
        self.count = [0] * n_params

    def call(self, flags, skipped):
        """one step() with these requires_grad flags; skipped: the guard found a non-finite trainable gradient"""
        for i, f in enumerate(flags):
            if f and not skipped:
                self.count[i] += 1
        return list(self.count)
