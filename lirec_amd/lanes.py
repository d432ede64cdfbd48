"""The train step's side streams and the state handed over between them: one ``StepLanes`` per model (``model.lanes``; DESIGN 4.4,
"Lanes").  Nothing here imports the model: a stand-in model builds one around a lane of its own."""
from __future__ import annotations

import collections
import ctypes as C

import torch

from . import ops
from .config import opt

# ONE lane per (device, priority, index) for the whole process, not one per model or recorded step: HIP deals streams onto a few
# hardware queues in creation order, and a stream made for the n-th object of a run has shared a queue with the step's own -- the
# "concurrent" lane then runs in line with the step (a fourth model's lane 0: 1.43 -> 2.10 ms/step; a staging lane: 0.86 -> 1.16).
_LANES = {}


# a side stream: the torch stream, its library context (own split-K scratch and GEMM core selection) or None, its raw handle
Lane = collections.namedtuple('Lane', 'stream ctx handle')


def lane(device, priority, index, scratch_bytes=0):
    """the process-wide lane (device, priority, index), made on first use; ``scratch_bytes``: with a library context of its own"""
    key = (str(device), priority, index)
    if key not in _LANES:
        stream, ctx = torch.cuda.Stream(device=device, priority=priority), None
        if scratch_bytes:
            ctx = ops.Context()
            with ctx:
                ops.ensure_scratch(device, scratch_bytes)
        _LANES[key] = Lane(stream, ctx, C.c_void_p(stream.cuda_stream))
    return _LANES[key]


class StepLanes:
    """Every flag is declared here once -- S: who sets it (a plain assignment), R: who reads it; a one-shot is read through the
    ``take_*`` method that clears it.  ``__slots__``: a misspelt flag raises instead of reading as False.  One optimiser per model:
    a second FusedAdam on the same model would share ``step_side_dev`` and replace ``side_ticket``."""
    __slots__ = ('sides', 'defer_join', 'unjoined', 'bucket0_on_side', 'bucket0_end', 'after_backward', 'fold', 'fold_applied',
                 'prestaged', 'atomic_step', 'step_side_dev', 'side_ticket')

    def __init__(self, sides=None):
        self.sides = dict(sides or {})  # index -> Lane: the weight-gradient lanes in use.  S: wgrad  R: join
        self.defer_join = False         # replayed steps leave lane 0 un-joined.  S: RecordedTrainStep  R: forward, may_defer
        self.unjoined = False           # lane 0 may still be running the last step.  S: backward, a replay  R: join, FusedAdam.step
        self.bucket0_on_side = False    # lane 0's own Adam launch wrote bucket 0 last.  S: FusedAdam.step, a replay  R: forward (one-shot), a replay
        self.bucket0_end = None         # end of the first gradient bucket in the flat buffers, cached.  S, R: take_after_backward
        self.after_backward = None      # one-shot (lane 0's handle, the stream backward ran on).  S: backward  R: FusedAdam.step
        self.fold = None                # one-shot (lirec_fused_adam args, hyper row, hyper map).  S: arm_first_layer_update  R: backward
        self.fold_applied = False       # one-shot: the last backward applied the folded update.  S: backward  R: FusedAdam.step
        self.prestaged = None           # one-shot: rows staged for the next forward.  S: RecordedTrainStep  R: forward
        self.atomic_step = False        # nothing runs between backward and step().  S: RecordedTrainStep  R: FusedAdam.step
        self.step_side_dev = None       # device int64[1], the Adam step as lane 0 counts it.  S: RecordedTrainStep  R: FusedAdam.step
        self.side_ticket = None         # device int32[1], lirec_adam_step_counted's arrival counter.  S: _ensure_state  R: FusedAdam.step

    def wgrad(self, device, which: int = 0):
        """weight-gradient lane ``which``, or None with ``opt.wgrad_side_stream`` off (priority 0: a lower one measured no better)"""
        if not getattr(opt, 'wgrad_side_stream', True):
            return None
        if which not in self.sides:
            self.sides[which] = lane(device, 0, which, (128 if which == 0 else 64) << 20)
        return self.sides[which]

    @staticmethod
    def staging(device):
        """the pipelined step's staging lane: the LOWEST priority there is (the pass is to fill what the step's own kernels leave)"""
        return lane(device, torch.cuda.Stream.priority_range()[0], 'stage')

    def join(self):
        """the current stream waits for lane 0 if a step left it un-joined; a flag test otherwise"""
        if self.unjoined and 0 in self.sides:
            ops.stream_wait(ops.current_stream_handle(), self.sides[0].handle)
        self.unjoined = False

    def params_written(self):
        """the parameters were written on the caller's stream: lane 0 is ordered behind it before it next reads them"""
        self.bucket0_on_side = False

    def take_bucket0_on_side(self):
        on_side, self.bucket0_on_side = self.bucket0_on_side, False
        return on_side

    def take_after_backward(self, offsets):
        """(lane 0's handle, end of bucket 0 in layout ``offsets``) when the caller is on the stream backward ran on; else None"""
        tag, self.after_backward = self.after_backward, None
        if tag is None or not getattr(opt, 'wgrad_side_stream', True) or not getattr(opt, 'adam_on_side_stream', True):
            return None
        side_h, main = tag
        if ops.current_stream_handle().value != main.value:
            return None
        if self.bucket0_end is None:
            from .parallel import bucket_ranges
            ranges, stages = bucket_ranges(offsets)
            self.bucket0_end = ranges[0][1] if (stages and stages[0] == 0 and len(ranges) > 1) else 0
        return (side_h, self.bucket0_end) if self.bucket0_end > 0 else None

    def take_fold(self):
        fold, self.fold = self.fold, None
        return fold or (None, None, None)

    def take_fold_applied(self):
        applied, self.fold_applied = self.fold_applied, False
        return applied

    def take_prestaged(self):
        pre, self.prestaged = self.prestaged, None
        return pre

    def may_defer(self, lane0, has_gate, has_ints, data_parallel, train):
        """may this backward leave lane 0 un-joined?  ("Lanes", invariant 1)"""
        return bool(self.defer_join and lane0 is not None and has_gate and has_ints and not data_parallel and train
                    and getattr(opt, 'adam_on_side_stream', True) and getattr(opt, 'wgrad_side_stream', True))
