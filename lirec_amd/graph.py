"""The train step issued without the Python loop: a command list recorded by the library.

A step of the hot path is ~25 kernel launches driven from Python (ctypes calls, a few torch allocations): about
0.5 ms of host work against ~1 ms of GPU work at B=64 on one MI355X.  Two things in a step change from one step to
the next and are normally passed to the kernels by value -- the dropout key (``opt.dropout_seed`` + number of training
forwards so far, ``lirec_amd/model.py:_begin_forward``) and Adam's step (bias corrections) -- so here both live in a small
device tensor that the step itself advances (``lirec_zero_count`` / ``lirec_counter_add``), and the kernels read them from
there (``lirec_dropout.seed_dev``, ``lirec_adam_step(step_dev)``).  A replay is therefore a NEW step: the same sequence of
dropout masks and parameter updates as the eager loop (tests/test_gpu_loops.py).

    g = RecordedTrainStep(model, loss, optimizer, batch)  # batch: device tensors, reused in place
    for _ in range(n):
        batch['features'].copy_(next_features)            # refill the static buffers, then
        loss_value = g.step()                             # device tensor [1]; no host sync

``RecordedTrainStep`` (what bench.py uses, with and without data parallelism): the library records the launches of one
ordinary eager step and re-issues them from C -- the eager loop's kernel timeline for ~0.1 ms of host time.  (Rounds 1-2
also carried a captured-hipGraph form of the step; its replay was slower on the GPU than the launches it was captured from
-- 10-20 us at every fork / join -- and it is gone: DESIGN 4.5.)
The reference has no counterpart (it is a plain eager PyTorch loop, mlp/train.py:57-63).
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import LirecError
from .config import opt


class _MarkingSync:
    """Stands in for the model's GradSync during the recorded (and really executed) data-parallel step: everything goes
    to the real one, and the positions in the command list where a bucket's all-reduce is issued and where Adam waits
    for one are noted."""

    def __init__(self, real, marks):
        self.real, self.marks = real, marks
        self.ranges, self.stages, self.world = real.ranges, real.stages, real.world

    def bucket_ready(self, stage, also=None):
        if self.real.world == 1 or stage not in self.real.stages or stage in self.real.launched or stage in self.real.reduced:
            return
        self.real.bucket_ready(stage, also=also)
        self.marks.append((ops.CommandList.mark(), 'reduce', stage, also))

    def wait_each(self):
        for s in self.stages:
            self.bucket_ready(s)
        pending, self.real.pending, self.real.launched = self.real.pending, [], set()
        self.real.reduced = set()
        for stage, work, via in pending:
            L = self.real.early_stream(stage, via)
            if work is not None:
                if L is not None:
                    with torch.cuda.stream(L):
                        work.wait()
                else:
                    work.wait()
            self.marks.append((ops.CommandList.mark(), 'wait', stage, L))
            self._cur = L
            yield self.ranges[self.stages.index(stage)] + (L,)
        self._cur = None

    def wait(self):
        for _ in self.wait_each():
            pass

    def my_slice(self, lo, hi):
        return self.real.my_slice(lo, hi)

    def grad_slice(self, g, lo, hi):
        return self.real.grad_slice(g, lo, hi)

    def gather_params(self, lo, hi):
        self.real.gather_params(lo, hi)
        self.marks.append((ops.CommandList.mark(), 'gather', (lo, hi), getattr(self, '_cur', None)))

    def finish_gathers(self):
        self.real.finish_gathers()
        self.marks.append((ops.CommandList.mark(), 'finish', None, None))

    sharded = property(lambda self: self.real.sharded)
    _launch_stream = property(lambda self: self.real._launch_stream)      # (FusedAdam: the early stream has a hyper-parameter table)
    real_world = property(lambda self: self.real.real_world)


_SENTINEL = 0x7FC0DEAD      # (as int32 bits) a quiet NaN with a payload no arithmetic produces


def _fill_sentinel(g):
    g.view(torch.int32).fill_(_SENTINEL)


def _overwrite_coverage(model, g) -> bool:
    """After a backward in overwrite mode on a buffer ``_fill_sentinel`` filled: was every PARAMETER element written?  Elements
    still holding the sentinel (unwritten parameters -- their gradient is 0 -- and the alignment gaps) are zeroed; a genuine NaN
    gradient (divergence) has another payload and stays, as it would in the eager loop.  One device reduction, one host sync.
    A FROZEN parameter (requires_grad False) needs no writer -- nothing reads its gradient: its elements count like the gaps."""
    mask = getattr(model, '_param_elem_mask', None)
    flags = tuple(p.requires_grad for p in model._plist)
    if mask is None or mask.device != g.device or mask.numel() != g.numel() or getattr(model, '_param_elem_mask_flags', None) != flags:
        mask = torch.zeros(g.numel(), dtype=torch.bool, device=g.device)
        live = {n for (n, _), f in zip(torch.nn.Module.named_parameters(model), flags) if f}
        for n, (off, k) in model._offsets.items():
            if n in live:
                mask[off:off + k] = True
        model._param_elem_mask, model._param_elem_mask_flags = mask, flags
    unwritten = g.view(torch.int32) == _SENTINEL
    covered = not bool((unwritten & mask).any())
    g.masked_fill_(unwritten, 0.0)
    return covered


def checked_overwrite_step(model, loss, optimizer, batch):
    """One ordinary train step on ``batch`` (eager launches, dropout key and Adam step by value) whose weight gradients OVERWRITE a
    gradient buffer pre-filled with a sentinel NaN instead of accumulating into a zeroed one -- the coverage check of the overwrite mode
    (``lirec_set_grad_overwrite``) done on a step the caller was going to take anyway.  Returns (ok, loss): ``ok`` = every
    parameter was written by exactly one gradient launch, i.e. a ``RecordedTrainStep(..., overwrite=True)`` of this model on batches
    of this layout may skip the zeroing pass.  The step itself is a correct step either way (an unwritten parameter's gradient
    is 0), bit-identical to the accumulate form."""
    if not bool(getattr(ops, 'set_grad_overwrite', None)) or getattr(model, 'grad_sync', None) is not None:
        optimizer.zero_grad()
        lv = loss(model(batch), batch)
        lv.backward()
        optimizer.step()
        return False, lv
    g = model.flat_grads(attach=True)
    _fill_sentinel(g)
    lv = loss(model(batch), batch)
    if getattr(lv, '_direct', None) is None:
        # (the overwrite switch is per calling thread: a backward through the autograd engine's thread would not see it)
        g.zero_()
        lv.backward()
        optimizer.step()
        return False, lv
    ops.set_grad_overwrite(True)
    try:
        lv.backward()
    finally:
        ops.set_grad_overwrite(False)
    g = model.flat_grads(attach=False)
    ok = _overwrite_coverage(model, g) and ops.grad_overwrite_conflicts() == 0
    optimizer.step()
    return bool(ok), lv


def _inside(blob, t) -> bool:
    """does tensor ``t`` lie inside the device buffer ``blob``?"""
    if not (torch.is_tensor(blob) and torch.is_tensor(t) and t.is_cuda):
        return False
    lo = blob.data_ptr()
    return lo <= t.data_ptr() <= lo + blob.numel() * blob.element_size() - t.numel() * t.element_size()


def _check_ids_in_blob(b, ids, who):
    """a batch of a resident block store: the recorded launches read its sample ids through their ADDRESS -- a refill of the batch's
    buffer reaches them only when the list lives inside that buffer; anywhere else every replay would read the recording batch's
    ids again"""
    if not _inside(b.get('_dev_blob'), ids):
        raise LirecError('%s: the block-store batch\'s clip_ids do not lie inside the batch\'s own buffer '
                         '(_dev_blob): a replay would keep reading the ids of the recording batch -- take the batch '
                         'from BlockLoader, or run the eager step' % who)


class RecordedTrainStep:
    """The train step as a command list recorded by the library while one ordinary eager step runs, then re-issued from
    C: the eager loop's launches on the eager loop's streams (so its kernel timeline: the weight-gradient side stream
    overlaps as it does there, no graph-node dependencies), for the host cost of one C loop.  On one MI355X the eager
    loop takes 0.9 ms of host time per 1.05 ms step, a hipGraph replay of the same step 1.13 ms; a replayed list takes
    the eager loop's GPU time and ~0.1 ms of host time.

    Works with and without data parallelism: with ``lirec_amd.parallel.DataParallel`` applied, the gradient reductions (and the parameter all-gathers of the sharded update)
    are issued from Python at the recorded positions between two stretches of the list (they are ordinary eager RCCL
    calls).  ``batch`` must hold device tensors that are refilled in place; every tensor the step allocates is kept
    alive by this object; call ``step()`` with the stream current that was current at construction.  The recorded step
    is a real step (every rank must construct this object at the same point of its program).
    """

    def __init__(self, model, loss, optimizer, batch, warmup: int = 2, next_batch=None, overwrite=None, draw=None):
        """``next_batch`` (a SECOND set of device buffers, single GPU, resident fp32 features): the input pipeline form.  Steps
        alternate between the two buffer sets, and each step stages the layer-1 operand rows of the OTHER set -- the batch the
        next step runs on -- on a stream of its own beside its backward (``model.prestage``): the rows do not depend on the
        weights, and the backward is MFMA-bound while the staging pass is HBM-bound.  Refill the set a step has just run on
        before the next call (it is the one the call after next reads); the set the next call steps on must already be
        filled -- its rows are staged DURING the current call.  Same numbers as the plain form, bit for bit.
        ``draw`` (a callable; plain single-GPU form): library launches that FILL ``batch``'s buffers, issued -- and recorded -- at the
        head of the list, in front of the step's first launch: every replay then draws its own batch (a resident block store:
        ``BlockLoader.collate_at``, lirec_collate_fields_at at a device cursor) and the host calls ``step()`` and nothing else.  The
        recording step runs them too: they must write the recording batch's own values."""
        if not model.training:
            raise ValueError('RecordedTrainStep records a TRAIN step: call model.train() first')
        for b in (batch, next_batch):
            f = b.get('features') if isinstance(b, dict) else None
            if torch.is_tensor(f) and f.requires_grad:
                # (a replay re-issues the recorded launches and returns no autograd graph: the features' gradient would be dropped)
                raise LirecError('RecordedTrainStep: the batch features require grad -- a recorded step computes no input gradient; '
                                 'run the eager step (model(batch) -> loss -> backward) instead')
            pcs = b.get('feature_pieces') if isinstance(b, dict) else None
            if isinstance(pcs, dict) and any(torch.is_tensor(pcs.get(k)) and pcs[k].requires_grad for k in ('clip', 'track')):
                # (likewise for piece tables that require grad: a replay would drop their gradient)
                raise LirecError('RecordedTrainStep: the batch\'s piece tables require grad -- a recorded step computes no input '
                                 'gradient; run the eager step (model(batch) -> loss -> backward) instead')
            ids = getattr(f, 'clip_ids', None)
            if ids is not None and next_batch is not None:
                # (two buffers would be two id slots, but the form's bit-identity test over such batches did not pass: DESIGN 4.n)
                raise LirecError('RecordedTrainStep(next_batch=...): the input-pipeline form is not built over block-store batches -- '
                                 'record the plain form')
            if ids is not None:
                _check_ids_in_blob(b, ids, 'RecordedTrainStep')
        if draw is not None and (next_batch is not None or getattr(model, 'grad_sync', None) is not None):
            raise ValueError('RecordedTrainStep(draw=...): the plain single-GPU form')
        self.model, self.loss, self.optim, self.batch, self.draw = model, loss, optimizer, batch, draw
        self._check_draw()
        self.lanes = model.lanes       # (lirec_amd.lanes.StepLanes: the side streams and the state handed over between them)
        self.batches = [batch, next_batch] if next_batch is not None else [batch]
        self.sync = getattr(model, 'grad_sync', None)
        if next_batch is not None and self.sync is not None:
            raise ValueError('RecordedTrainStep(next_batch=...): single-GPU form')
        # (what the optimiser's route is not recorded with -- FusedAdam.route: accumulation in the input-pipeline form, under data
        #  parallelism or on the norm route; the norm route under data parallelism -- is refused here, with the other argument checks:
        #  before anything of the optimiser or the device is touched)
        refuse = optimizer.route(pipelined=next_batch is not None).refuse
        if refuse is not None:
            raise LirecError(refuse)
        self.accum = optimizer.accumulate_steps
        self.win, self.overwrite, self.fused, self.defer = None, False, False, False
        dev = model.flat_params().device
        optimizer._ensure_state()
        optimizer.fold_if_due()           # (skipped steps of another frozen set, or of a guard since switched off: while the step is by value)
        # [forward calls (the dropout key's offset), Adam step, Adam step AS LANE 0 COUNTS IT]: the first two are advanced by the step's
        # first launch; the third by lane 0's own Adam launch, which under deferral may still run when the next step begins
        self.state = torch.tensor([model._fwd_train_calls, optimizer._step, optimizer._step], dtype=torch.int64, device=dev)
        # Gradient accumulation (FusedAdam.accumulate_steps = k > 1): the list re-issues the same launches every micro-step, so the
        # hold / apply decision lives beside ``state`` in device memory -- the WINDOW BLOCK of lirec_accum_begin, [phase, hold flag,
        # ticket, -], which the step's head launch advances and the update's launches read (ops.adam_hold).  Constructed at any
        # phase of a window: the block starts from the optimiser's host phase.
        if self.accum > 1:
            self.win = torch.tensor([optimizer.accum_phase, 0, 0, 0], dtype=torch.int64, device=dev)
        try:
            self._record(model, loss, optimizer, batch, warmup, next_batch, overwrite, dev)
        except BaseException:
            # (a failed recording leaves the eager loop's state behind: device-side counters detached, deferral off and the lane
            #  joined -- DESIGN 4.4, "Lanes")
            self.release()
            raise

    def _record(self, model, loss, optimizer, batch, warmup, next_batch, overwrite, dev):
        self._attach_counters()
        self.loss_out = torch.zeros(1, dtype=torch.float32, device=dev)
        self.stream = torch.cuda.current_stream()
        # The step is issued as a unit, so its weight gradients may OVERWRITE the flat gradient buffer instead of accumulating
        # into a freshly zeroed one (lirec_set_grad_overwrite): the 76 MB zeroing pass at the head of every step goes away.
        # Valid when every parameter gets exactly one gradient launch per step -- checked here, once, on a real step: the last
        # warm-up step runs in that mode on a buffer pre-filled with NaN; any NaN left after backward names a parameter nobody
        # wrote (its gradient is then 0, the step stays correct), and the library counts the buffers that were handed to MORE
        # than one gradient launch (lirec_grad_overwrite_conflicts): either way the mode stays off.  Single GPU only (a bucket's reduction
        # must not see a half-checked buffer).
        # (``overwrite``: the caller has run the check itself -- checked_overwrite_step on an earlier batch of this layout -- and
        #  passes its verdict: lirec_amd.train records with no warm-up step of its own)
        # (gradient accumulation IS the accumulate mode of the weight-gradient kernels: never the overwrite mode -- ``may_overwrite`` --
        #  and therefore -- `defer` below needs it -- never a deferred side join: every micro-step joins lane 0 before it ends, so the
        #  head launch of the next one rewrites the window's hold flag behind every launch that read it)
        may_overwrite = self.sync is None and optimizer.route().may_overwrite
        self.overwrite = bool(overwrite) if (overwrite is not None and may_overwrite) else False
        self.mid, self.parity, self.pre = None, 0, [None, None]
        # (warmup = 0: the caller has already run eager steps of this model -- lirec_amd.train records in the middle of an epoch,
        #  every batch being stepped on exactly once -- so the recording step is the only step taken here; the gradient-overwrite
        #  mode, which is checked on a warm-up step, then stays off)
        nwarm = max(int(warmup), 0)
        for w in range(nwarm):                     # lazy things happen here: scratch registered, side stream made, pools grown
            self._one_step(check=(w == nwarm - 1 and may_overwrite and overwrite is None and bool(getattr(ops, 'set_grad_overwrite', None))))
            self._advance_host()
        # The step is issued as a unit, so the update of the first-layer parameters -- the last gradients backward finishes -- is
        # folded into the launch that finishes them, which also keeps a q32b copy of the new weights for the next forward (no
        # separate Adam pass over that bucket, no staging of W1): FusedAdam.arm_first_layer_update.  Single GPU, layer 1 on the
        # q32b kernels (seen on the steps taken so far), and the optimiser's route: the first layers folded, or frozen altogether --
        # nothing writes them, the shadow stays current.  ('ordinary': the update writes no shadow, the forward stages the weights.)
        route = optimizer.route()
        self.fused = bool(getattr(opt, 'fuse_dw1_adam', True) and getattr(model, 'last_layer1_planes', False)
                          and getattr(model, '_has_ints', False) and getattr(model, '_has_ctx', False)
                          and hasattr(model, 'refresh_w1q') and route.first != 'ordinary')
        if self.fused:
            self.fused = model.refresh_w1q()
        # (does the recorded forward read the q32b shadow of the first-layer weights?  step() rebuilds a stale one before it replays)
        self._shadow_w1 = bool(self.fused and getattr(model, '_w1q_valid', False))
        # (did the recorded forward stage the gate's weights on lane 0 WITHOUT waiting for this stream -- bucket0_on_side at recording
        #  time?  step() then orders the lane behind this stream itself whenever something else has written the parameters since)
        self._side_unordered = False
        torch.cuda.synchronize()
        self.marks = []
        # Deferral ("Lanes"): needs the overwrite mode -- no zeroing pass over gradients the deferred update still reads --
        # and a route that updates on lane 0
        self.defer = bool(self.overwrite and getattr(opt, 'defer_side_join', True) and route.lane0)
        self.lanes.defer_join = self.defer
        if self.sync is not None:
            model.grad_sync = _MarkingSync(self.sync, self.marks)
        try:
            with ops.keep_allocations() as kept:
                if next_batch is not None:
                    # the rows of the first batch, staged here once (eagerly); from then on every step stages the other set's
                    self._pre_lane = self.lanes.staging(dev)
                    self.pre[0] = model.prestage(self.batches[0])
                    self.pre[1] = model.prestage(self.batches[1], advance=1)
                optimizer.sync_hyper()              # (a command list never contains a write to the hyper-parameter tables)
                ops.CommandList.begin()
                try:
                    if self.draw is not None:
                        self.draw()
                        if ops.CommandList.mark() < 1:
                            raise RuntimeError('RecordedTrainStep(draw=...): the callable issued no library launch')
                    self._one_step(k=0)
                    if next_batch is not None:
                        self._advance_host()
                        self.mid = ops.CommandList.mark()
                        self._one_step(k=1)
                finally:
                    self.cmds = ops.CommandList.end()
        finally:
            model.grad_sync = self.sync
        self._kept = kept
        self._hyper = self.hyper_key(optimizer)        # (baked into the recorded Adam launches by value: step() refuses a replay with others)
        self._gemm_mode = ops.get_gemm_mode()          # (the recorded launches ARE this core's kernels, reading its operand forms)
        self._advance_host()             # (``marks`` holds entries under data parallelism only: _MarkingSync wrote them)
        self._loss_outs = getattr(self, '_loss_outs', [self.loss_out])

    def _attach_counters(self):
        """the kernels read the dropout key's offset and the Adam step (the caller's and the side stream's count) from ``state``"""
        self.model._seed_dev, self.optim._step_dev = self.state[0:1], self.state[1:2]
        self.lanes.step_side_dev = self.state[2:3]
        if self.win is not None:
            self.optim._win_dev = self.win       # (the window of an accumulating step: decided on the device from here on)
        if hasattr(self.loss, '_sample_key'):
            self.loss._sample_calls = self.model._fwd_train_calls
            self.loss._seed_dev = self.state[0:1]

    def _one_step(self, check: bool = False, k: int = 0):
        over = self.overwrite or check
        batch = self.batches[k]
        pipelined = len(self.batches) == 2 and self.pre[k] is not None
        if check:
            _fill_sentinel(self.model.flat_grads(attach=True))
        # (+ this step's dropout key and Adam step, same launch; overwrite mode: the counters alone.  The side stream's part of Adam does
        #  not read this counter -- it counts the step itself, state[2] -- so nothing of the previous step is still looking at it here)
        if pipelined:
            # this batch's rows were staged during the previous step, on the staging stream: the step's stream joins it -- BEFORE
            # the launch that advances the dropout key: the staging pass derives this step's key from the device counter as it finds
            # it, workgroup by workgroup, and a low-priority pass that is still running when the next step begins would otherwise
            # make part of its keep bytes with the key after next (tests: ..._with_a_lagging_staging_stream_...)
            main, s3 = ops.current_stream_handle(), self._pre_lane.handle
            ops.stream_wait(main, s3)
        if self.accum > 1:
            # (accumulating: lirec_accum_begin in the place of lirec_zero_count -- the key every micro-step, the Adam step on the
            #  apply step, the zeroing pass where a window opens)
            self.optim.begin_micro_step(self.state)
        else:
            self.optim.zero_grad(counters=(self.state, [1, 1]), zero=not over)
        if pipelined:
            # ... and the forward is told where they are
            self.lanes.prestaged = self.pre[k]
            # ... and the OTHER buffer set's rows -- the next step's -- are staged beside this whole step (from its start: measured
            # best; beside the gate or behind the loss were slower, HISTORY round 4)
            ops.stream_wait(s3, main)
            with ops.on_stream(s3):                 # (the staging STREAM; this thread's own library context)
                self.pre[1 - k] = self.model.prestage(self.batches[1 - k], into=self.pre[1 - k], advance=0)
        if ops.CommandList.mark() >= 0 and k == 0:
            self._side_unordered = self.lanes.bucket0_on_side
        out = self.model(dict(batch))                # the model re-binds x['features'] (mlp/model.py:272)
        lv = self.loss(out, batch)
        # The recorder is thread-local: backward is recorded only when loss.backward() takes the direct path ON THIS THREAD
        # (lirec_amd.model._LossValue).  Through the autograd engine -- a wrapped or rescaled loss -- the hand-written backward
        # would run on the engine's thread, unrecorded, and every replay would update the parameters with zero gradients.
        recording = ops.CommandList.mark() >= 0
        if recording and getattr(lv, '_direct', None) is None:
            raise RuntimeError('RecordedTrainStep: loss.backward() would go through the autograd engine (the loss is not the '
                               'tensor the loss module returned, or its logits did not come straight from the model); the '
                               'backward launches cannot be recorded -- use the eager loop for this loss')
        before = ops.CommandList.mark()
        if self.fused and not check:
            self.optim.arm_first_layer_update()
        if over:
            ops.set_grad_overwrite(True)
        try:
            lv.backward()
        finally:
            if over:
                ops.set_grad_overwrite(False)
        if recording and ops.CommandList.mark() <= before:
            raise RuntimeError('RecordedTrainStep: backward issued no library launch on the recording thread')
        if check:
            # (unwritten elements -- alignment gaps, and, mode refused, parameters without a gradient launch -- are zeroed)
            if _overwrite_coverage(self.model, self.model.flat_grads(attach=False)):
                # ... and no buffer was the target of two launches (the second would have wiped out the first's share)
                self.overwrite = ops.grad_overwrite_conflicts() == 0
        # (nothing runs between this step's backward and its update: lane 0's share of Adam need not wait for backward's tail)
        self.lanes.atomic_step = not check
        try:
            self.optim.step()
        finally:
            self.lanes.atomic_step = False
        self.loss_out = lv.detach().reshape(-1)[:1]
        if len(self.batches) == 2 and ops.CommandList.mark() >= 0:
            self._loss_outs = (getattr(self, '_loss_outs', None) or [None, None])
            self._loss_outs[k] = self.loss_out

    def _advance_host(self):
        """Host mirrors of the device counters (checkpoints, switching back to the eager loop)."""
        self.model._fwd_train_calls += 1
        # (accumulating: the phase moves every micro-step; step, lags and the average's count on the apply step only -- the host
        #  knows which it was without reading the device: the phase is a function of the number of calls)
        applied = self.optim._advance_window() if self.accum > 1 else True
        if applied:
            self.optim._step += 1
            self.optim._opt_called = True           # (torch's lr_scheduler: an optimiser step HAS been taken -- no order warning)
            self.optim._advance_lags()              # (frozen parameters sat this update out, as in the eager step())
            self.optim._advance_ema()               # (the host count behind ema_updates(); skipped steps come off on the device's word)
        if hasattr(self.loss, '_sample_key'):
            self.loss._sample_calls += 1

    @staticmethod
    def hyper_key(optimizer):
        """the optimiser hyper-parameters a recorded step carries BY VALUE (lirec_adam_step's arguments) -- and, when any
        parameter is frozen or behind, the requires_grad flags and the trainable parameters' lags: they decided which launches
        were recorded and are in the recorded lirec_adam_step_ranges tables (FusedAdam.frozen_key)"""
        g = optimizer.param_groups[0]
        if hasattr(optimizer, 'resolve_device_hyper'):
            optimizer.resolve_device_hyper()      # (a group made decoupled since: the table route, i.e. another key -- or a ValueError)
        if getattr(optimizer, 'device_hyper', False):
            # (the hyper-parameters live in device tables the recorded launches hold by ADDRESS -- FusedAdam.sync_hyper writes what
            #  changed in front of a replay --; what is baked in is which group a range reads: the membership)
            key = (('device_hyper', optimizer.group_membership()), float(getattr(optimizer, 'grad_scale', 1.0)))
        else:
            key = (float(g['lr']), tuple(float(b) for b in g['betas']), float(g['eps']), float(g['weight_decay']), float(getattr(optimizer, 'grad_scale', 1.0)))
        frozen = optimizer.frozen_key() if hasattr(optimizer, 'frozen_key') else ()
        key = key + (frozen,) if frozen else key
        # (gradient clipping: whether the norm launches and the clipped Adam kernels were recorded, and the bound the recorded
        #  lirec_clip_finalize carries by value -- the coefficient itself is computed anew by every replay.  Off: today's key.)
        clip = getattr(optimizer, 'max_grad_norm', None)
        key = key + (('max_grad_norm', float(clip)),) if clip else key
        # (the guard: whether the guard finalize and the guarded Adam kernels were recorded.  Off: today's key.)
        key = key + (('skip_nonfinite', True),) if getattr(optimizer, 'skip_nonfinite', False) else key
        # (the weight average: whether the lirec_ema_step launches were recorded, and the weight they carry by value.  Off, or an
        #  optimiser without one: today's key.)
        ema = getattr(optimizer, 'ema_decay', None)
        key = key + (('ema_decay', float(ema)),) if ema is not None else key
        # (gradient accumulation: the head launch and the hold gate carry k by value.  Off (1): today's key.)
        k = int(getattr(optimizer, 'accumulate_steps', 1))
        return key + (('accumulate_steps', k),) if k > 1 else key

    def _check_core(self):
        if ops.get_gemm_mode() != self._gemm_mode:
            raise RuntimeError('RecordedTrainStep: recorded under GEMM mode %d, the library is in mode %d now -- the recorded launches are '
                               'the other core\'s kernels and read its operand forms (the shadow of the first-layer weights is q16c in the '
                               'single-pass mode, q32b otherwise): set the mode back, or release() and record again'
                               % (self._gemm_mode, ops.get_gemm_mode()))
        f = self.batch.get('features') if isinstance(self.batch, dict) else None
        if getattr(f, 'clip_ids', None) is not None and not getattr(opt, 'layer1_planes', False):
            # (the model refuses such a batch without the flag; a replay never asks the model)
            raise LirecError('RecordedTrainStep: recorded on a block-store batch, which the gathered q32b layer-1 kernels alone read '
                             '(opt.layer1_planes) -- the flag is off now: set it back, or release()')

    def _check_draw(self):
        """A list that draws its own batch leaves the host nothing to read of that batch in front of the replay: a loss with such
        work (``before_replay``: the cross-entropy loss's int32 label copies) would convert the PREVIOUS batch's labels."""
        if self.draw is not None and hasattr(self.loss, 'needs_before_replay') and self.loss.needs_before_replay():
            raise LirecError('RecordedTrainStep(draw=...): %s reads the batch on the host\'s side in front of every replay '
                             '(before_replay), i.e. before the list has drawn it -- record without draw= and fill the batch '
                             'before step()' % type(self.loss).__name__)

    def step(self):
        """Re-issue the recorded step; returns the loss as a device tensor (no synchronisation)."""
        self._check_draw()
        if self.hyper_key(self.optim) != self._hyper:
            raise RuntimeError('RecordedTrainStep: the optimiser\'s hyper-parameters changed since the step was recorded (%s -> %s); the '
                               'recorded Adam launches carry them by value -- release() this object and record a new one (a learning-'
                               'rate schedule: once per change)' % (self._hyper, self.hyper_key(self.optim)))
        self._check_core()
        if getattr(self.optim, 'device_hyper', False):
            # (what param_groups holds now -- a scheduler's step, a changed weight decay -- goes to the tables the recorded Adam
            #  launches read, each on the stream that reads it; no launch when nothing changed)
            import ctypes as C
            self.optim.sync_hyper(main=C.c_void_p(self.stream.cuda_stream))
        # The recorded forward reads the weights' q32b forms the recorded updates keep current.  Anything else that changed the
        # parameters since the last replay -- load_state_dict, an eager optimizer.step() without release() -- has marked them stale
        # (host flags): rebuild them from the parameters as they are now, on this stream, before the replay reads them.
        if self.fused and self._shadow_w1 and not getattr(self.model, '_w1q_valid', False):
            self.model.refresh_w1q()
        if self._side_unordered and not self.lanes.bucket0_on_side:
            lane = self.model._wgrad_lane()
            if lane is not None:
                ops.stream_wait(lane.handle, ops.current_stream_handle())
            self.lanes.bucket0_on_side = True       # (the replayed step's own Adam launch is the last writer again)
        if hasattr(self.loss, 'before_replay') and self.loss.needs_before_replay():
            # (what the recorded loss launch reads from buffers of the loss's own: under data parallelism the denominators of its
            #  valid-row means, all-reduced from the labels of the batch as it is NOW -- a collective, on every rank's replay; the CE
            #  loss's int32 label copies.  A no-op for the track losses on one GPU.)
            with torch.cuda.stream(self.stream):          # (ordered in front of the replay, whatever stream is current here)
                for b in self.batches if self.mid is None else [self.batches[self.parity]]:
                    self.loss.before_replay(b)
        if self.mid is not None:
            # the two recorded steps in turn (buffer set 0, buffer set 1)
            if self.parity == 0:
                self.cmds.replay(0, self.mid)
            else:
                self.cmds.replay(self.mid, -1)
            self.loss_out = self._loss_outs[self.parity]
            self.parity ^= 1
        elif not self.marks:
            self.cmds.replay(0, -1)
        else:
            sync, g, pos, works = self.sync, self.model.flat_grads(attach=False), 0, {}
            with torch.cuda.stream(self.stream):
                for at, kind, stage, also in self.marks:
                    if at > pos:
                        self.cmds.replay(pos, at)
                        pos = at
                    if kind == 'reduce':
                        lo, hi = sync.ranges[sync.stages.index(stage)]
                        if also is not None:
                            with torch.cuda.stream(sync._launch_stream):
                                works[stage] = sync.reduce(g, lo, hi)
                        else:
                            works[stage] = sync.reduce(g, lo, hi)
                    elif kind == 'wait':                    # (`also`: the early-update stream of this bucket, or None)
                        w = works.pop(stage, None)
                        if w is not None:
                            with torch.cuda.stream(also if also is not None else self.stream):
                                w.wait()
                    elif kind == 'gather':
                        with torch.cuda.stream(also if also is not None else self.stream):
                            sync.gather_params(*stage)
                    else:
                        sync.finish_gathers()
                self.cmds.replay(pos, -1)
        self._advance_host()
        self.lanes.unjoined = self.defer
        return self.loss_out

    def lag(self, command=None, ticks: int = 150000):
        """Diagnostics (the dependency fuzzer of the tests): from now on every replay holds the stream of recorded command
        ``command`` back by ``ticks`` of the 100 MHz clock in front of that command (None: off).  A correct step's bits do not
        depend on it: whatever crosses streams is ordered by a recorded event."""
        self.cmds.lag = None if command is None else (int(command), int(ticks))

    def flush(self):
        """The current stream waits for whatever a replayed step left running on the side stream (its first bucket's update): call
        before reading parameters / optimiser state with ordinary torch ops (an evaluation forward and state_dict() do it themselves)."""
        self.model.join_side_streams()

    def release(self):
        """Back to the eager loop: kernels take the key / step by value again."""
        self.model.join_side_streams()
        self.lanes.defer_join = False
        self.model._seed_dev = None
        self.optim._step_dev = None
        if self.win is not None:
            self.optim._win_dev = None      # (the window goes on from the host's phase: eager steps in between continue it)
        self.lanes.step_side_dev = None
        if hasattr(self.loss, '_sample_key'):
            self.loss._seed_dev = None
        if self.fused:
            self.model.invalidate_w1q()     # (eager steps update the weights without their q32b shadow)

    def resume(self):
        """After ``release()`` and any number of eager steps: the device-side counters take the host mirrors' values (one small
        copy) and the recorded list is valid again -- how a training loop steps on an odd-shaped batch in between
        (lirec_amd.train: the short last batch of an epoch)."""
        self._check_core()
        self.optim.fold_if_due()          # (the eager steps in between may have changed the frozen set: before the counters attach)
        self.state.copy_(torch.tensor([self.model._fwd_train_calls, self.optim._step, self.optim._step], dtype=torch.int64), non_blocking=False)
        if self.win is not None:
            # (the window's phase from the host mirror, as the counters: no device read in either direction)
            self.win.copy_(torch.tensor([self.optim.accum_phase, 0, 0, 0], dtype=torch.int64), non_blocking=False)
        self._attach_counters()
        if self.fused and not self.model.refresh_w1q():
            raise RuntimeError('RecordedTrainStep.resume(): the q32b shadow of the first-layer weights cannot be rebuilt')
        self.lanes.defer_join = self.defer
        self.lanes.params_written()             # (eager steps in between: whoever wrote the parameters last, order the side stream)


class RecordedEvalStep:
    """One FORWARD-ONLY iteration over a resident block store as a command list: the in-list draw (``draw``: ``BlockLoader.collate_at``
    -- the batch at the loader's device cursor, written into ``batch``'s own buffer, and the cursor's move), ``model(batch)`` under
    ``model.eval()`` and ``torch.no_grad()``, then ``tail(out, batch)`` -- whatever the caller does with the logits in LIBRARY launches
    (``testing()``: the loss, its accumulation and the device-side counters; ``predict()``: ``predict_clips_at``; both: the rows kept for
    after the loop and the move of the output cursor).  Recorded while it runs on a real batch, which counts; ``step()`` re-issues
    the list: one C loop in the place of ~20 launches driven from Python.

    Nothing a step reads is passed by value per call: the batch through the loader's cursor, the output rows through the caller's
    cursor word, the parameters through their addresses -- an evaluation forward reads neither the q32b shadow of the first-layer
    weights nor staged gate weights (both belong to training forwards), so the list computes what an eager forward at that moment
    would.  The object still lives for ONE call of ``testing()`` / ``predict()``: parameters, flags and scratch may change between
    two evaluations, and nothing here watches them.

    ``tail`` must not depend on a torch launch made from the batch (a dtype conversion, a host-side label copy): the list would not
    contain it and every replay would read the recording batch's values.  ``loss`` (optional) is asked as ``RecordedTrainStep`` asks
    it (``needs_before_replay``); the tail checks its own inputs (``in_batch``).  ``state``: device tensors the tail accumulates
    into -- a recording that raises puts back what they held, so the caller can run the batch eagerly."""

    def __init__(self, model, batch, draw, tail, loss=None, state=()):
        if model.training:
            raise ValueError('RecordedEvalStep records a forward-only step: call model.eval() first')
        f = batch.get('features') if isinstance(batch, dict) else None
        ids = getattr(f, 'clip_ids', None)
        if ids is None:
            raise LirecError('RecordedEvalStep: a batch of a resident block store (BlockLoader) is needed -- the list draws its own batches')
        _check_ids_in_blob(batch, ids, 'RecordedEvalStep')
        self.model, self.loss, self.batch = model, loss, batch
        self._check_draw()
        self.stream = torch.cuda.current_stream()
        self.cmds, self.out = None, None
        saved = [t.clone() for t in state]
        try:
            with torch.no_grad(), ops.keep_allocations() as kept:
                ops.CommandList.begin()
                try:
                    draw()
                    before = ops.CommandList.mark()
                    if before < 1:
                        raise RuntimeError('RecordedEvalStep: the draw issued no library launch')
                    out = model(dict(batch))              # the model re-binds x['features'] (mlp/model.py:272)
                    if ops.CommandList.mark() <= before:
                        raise RuntimeError('RecordedEvalStep: the forward issued no library launch on the recording thread')
                    self.out = tail(out, batch)
                finally:
                    self.cmds = ops.CommandList.end()
        except BaseException:
            # (a failed recording leaves the eager loop's state behind: the accumulators as they were, no list)
            for t, s in zip(state, saved):
                t.copy_(s)
            self.release()
            raise
        self._kept = kept
        self._gemm_mode = ops.get_gemm_mode()

    in_batch = staticmethod(_inside)

    def _check_draw(self):
        if self.loss is not None and hasattr(self.loss, 'needs_before_replay') and self.loss.needs_before_replay():
            raise LirecError('RecordedEvalStep: %s reads the batch on the host\'s side in front of every replay (before_replay), i.e. '
                             'before the list has drawn it -- run the eager loop' % type(self.loss).__name__)

    def step(self):
        """Re-issue the recorded iteration on the batch the loader's cursor names now (no synchronisation)."""
        if self.cmds is None:
            raise RuntimeError('RecordedEvalStep: released')
        self._check_draw()
        if self.model.training:
            raise RuntimeError('RecordedEvalStep: the model is in train mode -- the list holds an evaluation forward')
        if ops.get_gemm_mode() != self._gemm_mode or not getattr(opt, 'layer1_planes', False):
            raise RuntimeError('RecordedEvalStep: recorded under GEMM mode %d with opt.layer1_planes, the library is in mode %d now (flag %s) '
                               '-- the recorded launches are that core\'s kernels' % (self._gemm_mode, ops.get_gemm_mode(), getattr(opt, 'layer1_planes', False)))
        self.cmds.replay(0, -1)
        return self.out

    def release(self):
        """the list and everything it kept alive go (the stream has been told to run them first)"""
        if self.cmds is not None:
            self.cmds.destroy()
        self.cmds, self._kept = None, None


class EvalStepper:
    """The life of a ``RecordedEvalStep`` inside ONE call of ``testing()`` / ``predict()`` (``opt.record_eval``): the first batch of a
    layout runs eagerly (lazy allocations happen), the next one of that layout is recorded -- a real batch, run once --, every further
    one is a replay; a batch of another layout (the short last one, a singleton) runs eagerly in between, drawn by the loader's own
    call, the loader's cursor account kept right by the loader.  A recording that raises bars further attempts: the loop finishes
    eagerly.  ``replayed`` counts the replays."""

    def __init__(self, model, loader, loss=None, say=print):
        self.model, self.loader, self.loss, self.say = model, loader, loss, say
        self.step = self.layout = None
        self.seen, self.barred, self.replayed = set(), False, 0
        loader.stable_ids = True          # (asked for before the epoch is drawn: a list reads the epoch's ids at ONE address)

    @staticmethod
    def wanted(loader, world=1) -> bool:
        """``opt.record_eval`` over a BlockLoader in one process -- anything else is today's loop, with no complaint"""
        from .loader import BlockLoader
        return bool(getattr(opt, 'record_eval', False)) and isinstance(loader, BlockLoader) and world == 1

    def take(self, batch, tail, state=()):
        """(handled, batch): handled -- the batch was evaluated by the recording or by a replay and the caller does its host accounting
        only; else the caller runs ``batch`` (materialised, had it been left to a list that will not run) eagerly."""
        lay = tuple(batch.get('_layout', ())) if isinstance(batch, dict) else ()
        if self.step is not None and lay == self.layout and self.loader.last_in_list:
            try:
                self.step.step()
                self.replayed += 1
                return True, batch
            except Exception as e:
                self._give_up('replay', e)
        if self.loader.last_in_list:
            return False, self.loader.materialise(batch)
        if self.step is None and not self.barred and lay and lay in self.seen and self.loader.can_draw_last_in_list():
            loader, blob = self.loader, batch['_dev_blob']
            try:
                loader.cursor_to_last()
                self.step = RecordedEvalStep(self.model, batch, lambda: loader.collate_at(lay, blob), tail, loss=self.loss, state=state)
                self.layout = lay
                loader.bind(lay, blob, in_list=True)
                return True, batch
            except Exception as e:
                self._give_up('recording', e)
        if lay:
            self.seen.add(lay)
        return False, batch

    def _give_up(self, what, e):
        self.say('recorded evaluation step not used (%s): %s' % (what, str(e)[:160]))
        self.barred = True
        self.loader.unbind()
        self.loader.cursor_lost()
        if self.step is not None:
            self.step.release()
            self.step = None

    def close(self):
        """at the end of the call: the loader draws by its own calls again, the list goes"""
        self.loader.unbind()
        if self.step is not None:
            torch.cuda.current_stream().synchronize()      # (the buffers the list kept alive are still being read)
            self.step.release()
            self.step = None
