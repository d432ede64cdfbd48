"""Fused Adam over the model's flat parameter buffer.

Replaces ``torch.optim.Adam(model.parameters(), lr=opt.lr, weight_decay=opt.weight_decay)``
(mlp/model.py:599-601) -- 38 parameter tensors x 5 ATen ops each in the reference
(27 % of its CPU train step) -- with one HIP kernel launch over one
contiguous buffer (``lirec_adam_step``).  Same update rule (coupled L2 weight
decay, bias correction, eps outside the sqrt) and the same ``state_dict`` layout
(``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter, in ``model.parameters()``
order), so optimizer states of reference checkpoints load unchanged
(utils/util_functions.py:283-291).

Frozen parameters (``p.requires_grad_(False)``) are honoured as torch.optim.Adam honours a ``grad is None``: ``step()`` updates
exactly the parameters that require grad when it is called; a frozen one keeps its value and its moments bit for bit, and its
``state[p]['step']`` -- the number of updates IT has received -- stops.  That count is kept as a lag behind the global step
(``_lag``); the trainable parameters become ranges ``(offset, length, lag)`` of the flat buffers, and a stretch of an update
that is not simply one zero-lag range is one ``lirec_adam_step_ranges`` launch.  One difference from torch 1.1 (the
reference's pin), none from current torch: there ``zero_grad()`` zeroes a gradient instead of dropping it, so a parameter frozen
AFTER it has trained keeps being updated on a zero gradient (weight decay and its old momentum); here it stops.

Gradient clipping by global norm (``max_grad_norm``; ``torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)`` in front
of the step, norm type 2) happens on the device, inside the update: a reduction over the trainable ranges of the flat gradient
buffer (``lirec_grad_sq_partials`` / ``lirec_clip_finalize``) leaves the coefficient min(1, max_norm / (norm + 1e-6)) in device
memory and the Adam launches multiply it into the scale they apply to every gradient anyway (``lirec_set_adam_clip``) -- no pass
over the gradients, no host visit, so the recorded step and the sharded data-parallel update can clip too.  ONE DIFFERENCE FROM
TORCH: the gradients in the flat buffer -- every ``p.grad`` -- stay UNCLIPPED after the step (``clip_grad_norm_`` scales them in
place); whoever wants the clipped values multiplies by ``optimizer.clip_coef``.  The update itself is the same to one fp32 rounding
of the scalar: g (grad_scale coef) here, (g coef) grad_scale there.

Parameter groups (``param_groups=[{'params': [names or parameters], 'lr': ..., 'weight_decay': ...}, ...]``, at most 8) and
device-resident hyper-parameters (``device_hyper``): lr, betas, eps and weight_decay of every group live in a small table in device
memory that the Adam launches read (``lirec_adam_step_groups``; the folded first-layer update through
``lirec_set_adam_hyper_row``) instead of taking them by value.  ``self.param_groups`` is torch's list: a scheduler, or a loop that
assigns ``g['lr']``, changes the values and ``sync_hyper()`` -- called by ``step()`` and in front of every replay of a recorded
step -- sends what changed, one tiny launch per table.  ONE TABLE PER ISSUING STREAM (the caller's, the weight-gradient side
stream, the collectives' early stream), each written only on the stream that reads it: a replayed step leaves the side stream's
Adam launch of step t running into step t + 1, and a write from the main stream would hand part of that launch the next step's
values.  ``device_hyper=None`` is on with more than one group and off with one; off with one group is the by-value code path,
launch for launch.  The groups are fixed at construction (the flat layout is): ``add_param_group`` raises afterwards.

Decoupled weight decay -- AdamW -- per group (``decoupled_weight_decay``, torch's key: ``torch.optim.AdamW`` is
``torch.optim.Adam`` with it set): p is multiplied by (float)(1 - lr wd) in front of the step and the decay stays out of the
gradient, hence out of the moments and of a clipped norm's reach (the clip scales g only); a frozen parameter gets no decay.  The
flag is a TABLE value like lr (word 5 of a group's row): a decoupled group needs ``device_hyper`` -- ``None`` resolves to on with
any decoupled group, an explicit ``False`` with one is a ValueError -- ``sync_hyper()`` sends a change, a recorded step follows it.
The by-value launches know the coupled form only.  1 - lr wd is exactly 1 in fp32 when lr wd < 2^-25: with the reference's
defaults (3e-5 x 1e-5) decoupled decay does nothing, here as in torch's fp32 ``mul_``.  ``state_dict()`` goes to
``torch.optim.AdamW`` / ``torch.optim.Adam(decoupled_weight_decay=True)`` with the same groups and back.  Under ``device_hyper``
the first-layer update stays folded into the backward (``arm_first_layer_update``) when the first layers span SEVERAL groups --
weights that decay, biases that do not --: each parameter then reads the row of its own group (``lirec_set_adam_hyper_map``).

Skipping non-finite steps (``skip_nonfinite``, off by default; apex's ``noop_flag``, torch's ``_fused_adam(found_inf=)``): a step
whose TRAINABLE gradients hold a NaN or an Inf leaves parameters and moments bit for bit untouched and does not count as an update
for the bias corrections -- what a loop that calls ``step()`` only when the norm is finite gets -- decided on the device, with no
host visit, so the recorded step and the sharded data-parallel update have it too.  The step takes the clipped route whether or
not ``max_grad_norm`` is set (the norm's double sum of squares is non-finite exactly when a gradient element is; computed once for
both features), then one ``lirec_clip_finalize_guard`` that also counts, then the whole update inside ``ops.adam_guard``: no update
beside the tail of backward, no folded first-layer update.  ``found_nonfinite`` / ``skipped_steps`` are device views.  ACCOUNTING:
``_step`` (and a recorded step's device counter) count every call; the kernels subtract S = the device count of skipped steps.
Between two changes of the frozen set a trainable parameter has received ``_step - lag - S`` updates, a frozen one ``_step - lag``
(its lag advances every call); ``state_dict()`` reports exactly that.  Where the frozen set changes, or the guard is switched off
with steps skipped, the optimiser FOLDS S into ``_step`` and the frozen parameters' lags (one read of S, a synchronisation at a
rare event) -- legal only where the step is by value: at the top of an eager ``step()``, before a recording attaches its counters.
The gradients stay as backward left them, non-finite values included.

An exponential moving average of the weights (``ema_decay``, off by default; ``torch.optim.swa_utils.AveragedModel(model,
multi_avg_fn=get_ema_multi_avg_fn(decay))``, timm's ``ModelEmaV2``): ``optimizer.ema`` is a second flat buffer, a copy of the
parameters at the moment the average is switched on, and every APPLIED step is one ``ema.lerp_(p, 1 - decay)`` -- torch's bits
(``lirec_ema_step``).  The lerp of a stretch of the buffer is a library launch directly behind that stretch's Adam launch, on that
launch's stream: a recorded step contains it, the side stream's bucket and a rank's own slices are averaged where they are
updated, and on the guarded route the launch reads the flag, so a skipped step is no update of the average either.  The shadow
covers the WHOLE buffer (lerp(e, p) with e == p is e -- up to the sign of a zero: fmaf(w, +0, -0) is +0, in torch too --: a
parameter frozen from the start stays identical to its shadow, one frozen after it has trained keeps converging to its resting
value; the alignment gaps, zeros in both buffers, stay zeros).  ``ema_weights()`` evaluates with the average, ``ema_state_dict()``
is what a checkpoint keeps; ``state_dict()`` is unchanged.  timm's semantics; ``AveragedModel`` differs in its first update, which
copies: ``ema_reset()`` after the first step reproduces it.

Gradient accumulation (``accumulate_steps=k``, 1 = off by default): one update per k micro-batches with the stock loop --
``zero_grad()``, backward, ``step()`` -- unchanged.  ``accum_phase`` counts the micro-batches already in the open window, a pure
function of the number of ``step()`` calls.  ``zero_grad()`` zeroes only when the next micro-batch opens a window; calls 1 .. k-1 of
``step()`` ("hold") touch nothing -- parameters, moments, average, ``_step``, lags and the skipped count keep their bits, and
under data parallelism no bucket is reduced and nothing gathered (torch's ``no_sync``) --; call k ("apply") is one ordinary update
on the accumulated gradient times ``grad_scale / k`` (``ops.accum_scale``: folded into the scale every Adam launch applies anyway,
no pass over the gradients).  ``p.grad`` holds the UNSCALED SUM of the window so far (the clip's precedent: ``p.grad`` stays
unclipped).  Clip, guard, AdamW, groups, frozen parameters and the average act at the apply step on the accumulated gradient: the
norm is that of sum / k x grad_scale, a NaN anywhere in the window skips the window's update and counts ONE skipped step, the
average takes one lerp per applied window; ``state_dict()`` counts updates.  A checkpoint taken inside a window does not hold the
window's gradients in ``state_dict()``; ``window_state()`` / ``load_window_state()`` carry them (lirec_amd.train.TrainState).  In the eager loop the host takes the hold / apply decision; a recorded step re-issues the same launches every
micro-step, so there it lives in device memory (``_win_dev``, the window block of lirec_accum_begin; the update's launches under
``ops.adam_hold``) -- ``begin_micro_step`` is that step's head.

Per-parameter statistics (``param_stats()``, ``nonfinite_params()``; on demand -- no step issues them): gradient norm and largest
magnitude as the update sees them, weight norm, the size of the last applied Adam step against the weight and the counts of
non-finite elements, for every parameter, from one deterministic pass over the four flat buffers (``lirec_param_stats``: double
accumulation in a fixed order, no atomics, the same bits every call).  Single process only: under data parallelism the moments and
the reduced gradients live in slices, and a defined answer would need collectives.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C

import torch

from . import ops
from .config import opt


# The route of one update, FusedAdam.route() -- DESIGN 4.4, "The update's route".  hold: a host-side hold step, nothing is issued;
# norm / guard: the norm route (clip, guard) is in force / with the guard; window: the accumulation window is on the device; parallel:
# world > 1; lane0: bucket 0 may be updated on lane 0; first: the first layers in a step issued as a unit -- 'value' / 'row' / 'map'
# (folded into the backward: by value, reading one device row, through the per-parameter map), 'untouched' (frozen altogether) or
# 'ordinary'; may_overwrite: the weight gradients may overwrite the buffer; refuse: why the step cannot be recorded, or None
Route = collections.namedtuple('Route', 'hold norm guard window parallel lane0 first may_overwrite refuse')

# One parameter's row of ``ParamStats.host()``.  A column that was not asked for is None.
ParamStat = collections.namedtuple('ParamStat', 'grad_norm grad_absmax grad_nonfinite param_norm param_absmax param_nonfinite '
                                                'update_norm update_absmax update_nonfinite update_ratio')


class ParamStats:
    """What ``FusedAdam.param_stats()`` returns.  ``names``: every parameter in ``model.named_parameters()`` order; ``table``: device
    float64 [P, 9], row i the raw columns of lirec_param_stats for ``names[i]`` (sums of squares, unscaled maxima, counts; a group
    that was not asked for is 0 there) -- no synchronisation; ``flags``: per row, which groups were asked for (1 gradient,
    2 parameter, 4 update); ``scale``: what the update multiplies the gradients by; ``lrs``: each parameter's group's lr.
    ``host()``: ONE copy to the host, then {name: ParamStat}."""

    def __init__(self, names, table, flags, scale, lrs):
        self.names, self.table, self.flags, self.scale, self.lrs = list(names), table, list(flags), float(scale), list(lrs)

    def host(self):
        from ._lib import STAT_GRAD, STAT_PARAM, STAT_UPDATE
        rows = self.table.cpu().tolist()
        out = collections.OrderedDict()
        for name, row, f, lr in zip(self.names, rows, self.flags, self.lrs):
            g = (row[0] ** 0.5 * self.scale, row[1] * self.scale, int(row[2])) if f & STAT_GRAD else (None,) * 3
            p = (row[3] ** 0.5, row[4], int(row[5])) if f & STAT_PARAM else (None,) * 3
            u = (lr * row[6] ** 0.5, lr * row[7], int(row[8])) if f & STAT_UPDATE else (None,) * 3
            ratio = u[0] / p[0] if (u[0] is not None and p[0]) else None
            out[name] = ParamStat(*g, *p, *u, ratio)
        return out


class FusedAdam(torch.optim.Optimizer):
    MAX_GROUPS = 8                     # (LIREC_ADAM_MAX_GROUPS: the rows of a hyper-parameter table)

    @staticmethod
    def _check_values(lr, betas, eps, weight_decay):
        """the values torch.optim.Adam rejects, with its messages"""
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: {}'.format(lr))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: {}'.format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError('Invalid beta parameter at index 0: {}'.format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError('Invalid beta parameter at index 1: {}'.format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError('Invalid weight_decay value: {}'.format(weight_decay))

    def __init__(self, model, lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, max_grad_norm=None, param_groups=None,
                 device_hyper=None, amsgrad=False, decoupled_weight_decay=False, skip_nonfinite=False, ema_decay=None,
                 accumulate_steps=1):
        self.model = model
        self.lanes = getattr(model, 'lanes', None)       # (lirec_amd.lanes.StepLanes; None: every update on the caller's stream)
        params = list(model.parameters())
        self._names = [n for n, _ in model.named_parameters()]        # (in the order of model._plist)
        if amsgrad:
            raise ValueError('FusedAdam: amsgrad is not supported (the reference never sets it, mlp/model.py:599-601)')
        self._check_values(lr, betas, eps, weight_decay)
        # (amsgrad: part of torch.optim.Adam's param_groups since torch 1.1 -- the reference's pin -- so that an
        #  optimizer state_dict saved here has the keys a stock Adam expects, and the other way round)
        # (decoupled_weight_decay: torch.optim.Adam's key since torch 2.x -- what makes a group AdamW)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                        decoupled_weight_decay=bool(decoupled_weight_decay))
        if param_groups is None:
            super().__init__(params, defaults)
        else:
            super().__init__(self._resolve_groups(param_groups, params), defaults)
        for grp in self.param_groups:
            if grp.get('amsgrad'):
                raise ValueError('FusedAdam: amsgrad is not supported (the reference never sets it, mlp/model.py:599-601)')
            self._check_values(grp['lr'], grp['betas'], grp['eps'], grp['weight_decay'])
        self._layout_fixed = True      # (add_param_group from here on raises)
        gi = {id(p): i for i, grp in enumerate(self.param_groups) for p in grp['params']}
        self._group_of = {n: gi[id(p)] for n, p in zip(self._names, params)}          # parameter name -> index of its group
        many = len(self.param_groups) > 1
        if many and device_hyper is not None and not device_hyper:
            raise ValueError('FusedAdam: %d parameter groups need device_hyper (by value the launches carry one set of '
                             'hyper-parameters)' % len(self.param_groups))
        self._device_hyper_arg = None if device_hyper is None else bool(device_hyper)     # (None: left to default)
        self.device_hyper = many if device_hyper is None else bool(device_hyper)
        self._ranges_key = self._ranges = self._first = None
        self.resolve_device_hyper()    # (a decoupled group: on, or a ValueError for an explicit False)
        self._tables = {}              # issuing stream ('main', 'side', 'early') -> [device float32[64], the rows it last received]
        self._m = self._v = None
        self._step = 0
        self.grad_scale = 1.0          # 1/world_size after a summing all-reduce
        self._step_dev = None          # device int64[1]: the step kept on the GPU (lirec_amd.graph)
        self._lag = {}                 # parameter name -> updates it sat out frozen (missing = 0): state[p]['step'] = _step - lag
        self.max_grad_norm = max_grad_norm      # None / 0: no clipping; settable between steps (a recorded step is recorded again)
        self._clip_out = None          # device float32[4]: (clip coefficient, gradient norm, skipped?, -) of the last clipped / guarded step
        self.skip_nonfinite = bool(skip_nonfinite)      # settable between steps (a recorded step is recorded again)
        self._skipped_dev = None       # device int64[1]: S, the steps skipped since the last fold
        self._skipped_folded = 0       # skipped steps already folded into _step (skipped_total)
        self._guard_flags = None       # the requires_grad flags of the interval S counts in; None: no guarded step since the fold (S = 0)
        self._guard_now = False
        self._ema = None               # the flat shadow (allocated by _ensure_state once ema_decay is set; kept when it is switched off)
        self._ema_decay = self._ema_w = None
        self._ema_calls = 0            # steps issued with the average on since the count was last folded ...
        self._ema_skip_base = 0        # ... and skipped_total() at that moment: ema_updates() = done + calls - skipped since
        self._ema_done = 0
        self.ema_decay = ema_decay     # None: off; settable between steps (a recorded step is recorded again)
        self._accum_k, self._accum_phase = 1, 0
        self._win_dev = None           # device int64[4]: the window block while a recorded step holds the phase on the device (lirec_amd.graph)
        self.accumulate_steps = accumulate_steps      # settable between windows (a recorded step is recorded again)

    # -- gradient accumulation ------------------------------------------------------
    @property
    def accumulate_steps(self):
        return self._accum_k

    @accumulate_steps.setter
    def accumulate_steps(self, k):
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError('FusedAdam.accumulate_steps must be an integer >= 1, not %r' % (k,))
        if k != self._accum_k and self._accum_phase != 0:
            raise RuntimeError('FusedAdam.accumulate_steps changed in the middle of a window (%d of %d micro-batches taken): change it '
                               'after the step() that applies the window, or drop_window() first' % (self._accum_phase, self._accum_k))
        if k != self._accum_k and self._win_dev is not None:
            raise RuntimeError('FusedAdam.accumulate_steps changed while a recorded step holds the window on the device; release() '
                               'the recorded step first')
        self._accum_k = k
        self._hold_sync()

    @property
    def accum_phase(self):
        """host int: the micro-batches already in the open window, 0 .. accumulate_steps - 1 (0: the next one opens a window)"""
        return self._accum_phase

    @staticmethod
    def window_after(phase, k):
        """(phase after one more ``step()``, did that call apply?) -- the whole phase arithmetic: the call that finds k - 1
        micro-batches in the window applies and closes it"""
        return (0, True) if phase + 1 >= k else (phase + 1, False)

    def _advance_window(self):
        """one ``step()`` has been issued (the eager one, a replay: lirec_amd.graph); returns whether it applied"""
        self._accum_phase, applied = self.window_after(self._accum_phase, self._accum_k)
        self._hold_sync()
        return applied

    def drop_window(self):
        """forget the open window: its micro-batches are dropped, the next ``zero_grad()`` zeroes (what ``training()`` does with a
        partial window at its end).  Not while a recorded step holds the window on the device."""
        if self._win_dev is not None:
            raise RuntimeError('FusedAdam.drop_window(): a recorded step holds the window on the device; release() it first')
        self._accum_phase = 0
        self._hold_sync()

    def window_state(self):
        """the open accumulation window as a checkpoint keeps it (lirec_amd.train.TrainState; ``state_dict()`` does not hold it):
        {'phase', 'k', 'grads'} -- ``grads`` a host copy of the flat gradient buffer, the unscaled sum of the window's micro-batches
        so far, when the phase is not 0, else None.  The phase is the host's (a recorded step keeps its mirror current); the copy
        waits for the side stream and the device."""
        grads = None
        if self._accum_phase != 0:
            self._join_side()
            grads = self.model.flat_grads(attach=True).detach().cpu().clone()
        return self.window_state_from(self._accum_phase, self._accum_k, grads)

    @staticmethod
    def window_state_from(phase, k, grads):
        """``window_state()`` of a window at ``phase`` of ``k`` whose flat gradient buffer is the host tensor ``grads`` (kept as it
        is given; dropped at phase 0, where no window is open)"""
        return {'phase': int(phase), 'k': int(k), 'grads': grads if int(phase) != 0 else None}

    @torch.no_grad()
    def load_window_state(self, ws):
        """continue the window of ``window_state()``: the gradients back into the flat buffer, the phase set -- the next
        ``zero_grad()`` then leaves them alone and the next ``step()`` counts on from there.  Not under a recorded step."""
        if self._win_dev is not None:
            raise RuntimeError('FusedAdam.load_window_state(): a recorded step holds the window on the device; release() it first')
        phase, k = int(ws['phase']), int(ws['k'])
        if k != self._accum_k:
            raise ValueError('FusedAdam.load_window_state: the window was taken with accumulate_steps=%d, this optimiser has %d' % (k, self._accum_k))
        if not 0 <= phase < k or (phase != 0 and ws.get('grads') is None):
            raise ValueError('FusedAdam.load_window_state: phase %d of %d%s' % (phase, k, ' without the window\'s gradients' if phase else ''))
        if phase != 0:
            g = self.model.flat_grads(attach=True)
            if ws['grads'].numel() != g.numel():
                raise ValueError('FusedAdam.load_window_state: %d gradient elements, the model has %d' % (ws['grads'].numel(), g.numel()))
            self._join_side()
            g.copy_(ws['grads'].reshape(-1))
        self._accum_phase = phase
        self._hold_sync()

    def _hold_sync(self):
        """data parallelism: tell the gradient sync whether the NEXT backward belongs to a hold step -- its buckets are then not
        reduced (torch's no_sync, automatic); the apply step's backward reduces the accumulated local gradients"""
        sync = getattr(self.model, 'grad_sync', None)
        if sync is not None and hasattr(sync, 'hold'):
            sync.hold = self._accum_k > 1 and not self.window_after(self._accum_phase, self._accum_k)[1]

    def _scale(self):
        """what the update multiplies the gradient buffer by: ``grad_scale``, over k for the sum of a window"""
        return self.grad_scale if self._accum_k == 1 else ops.accum_scale(self.grad_scale, self._accum_k)

    def begin_micro_step(self, counters):
        """lirec_amd.graph, accumulating form: the head launch of a recorded micro-step in the place of ``zero_grad(counters=)`` --
        lirec_accum_begin on the window block: the dropout key's counter advanced every time, the Adam step (the caller's and
        lane 0's, which issues no update of its own here) on the apply step only, the gradient buffer zeroed when a window opens"""
        g = self.model.flat_grads(attach=True)
        ops.accum_begin(g, counters, [1, 0, 0], [0, 1, 1], self._win_dev, self._accum_k)

    # -- exponential moving average of the weights ----------------------------------
    @property
    def ema_decay(self):
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, decay):
        w = None if decay is None else ops.ema_weight(decay)      # (ValueError unless 0.5 < decay < 1)
        if (decay is None) != (self._ema_decay is None):
            if decay is None:
                self._ema_done, self._ema_calls = self.ema_updates(), 0
            else:
                self._ema_calls, self._ema_skip_base = 0, self.skipped_total()
        self._ema_decay, self._ema_w = (None if decay is None else float(decay)), w
        if decay is not None and self._m is not None:
            self._ensure_state()       # (switched on in the middle of a run: the shadow is the parameters as they are NOW)

    @property
    def ema(self):
        """the flat shadow (laid out as ``model.flat_params()``), or None while the average has never been on"""
        return self._ema

    def _ensure_ema(self, flat, force=False):
        """the shadow on the parameters' device: made as a copy of them, or re-made from its per-parameter views after a move"""
        if self._ema is not None and self._ema.device == flat.device and self._ema.numel() == flat.numel():
            return
        if self._ema is None and self._ema_decay is None and not force:
            return
        if ops.CommandList.mark() >= 0:
            raise RuntimeError('FusedAdam: the EMA shadow cannot be made while a step is being recorded; set ema_decay before')
        self._join_side()
        old = getattr(self, '_ema_views', None) if self._ema is not None else None
        self._ema = flat.clone()
        self._ema_views = {}
        for n, (off, k) in self.model._offsets.items():
            view = self._ema[off:off + k]
            if old is not None and n in old and old[n].numel() == k:
                view.copy_(old[n])
            self._ema_views[n] = view
        if old is None:
            self._ema_done, self._ema_calls, self._ema_skip_base = 0, 0, self.skipped_total()
        if flat.is_cuda:
            # (as for the moments in _ensure_state: the first lerp may run on another stream than the one that made the copy)
            torch.cuda.current_stream(flat.device).synchronize()

    def ema_updates(self):
        """the lerps applied to the shadow since it was last (re)initialised, as a host int: steps taken with the average on,
        less the ones the guard skipped (one read of the device count when a guard has been on: synchronises, as
        ``skipped_total()`` does)"""
        if self._ema_decay is None:
            return self._ema_done
        return self.ema_updates_at(self.host_cut(groups=False), self._read_skipped())

    @staticmethod
    def ema_updates_at(cut, skipped):
        """``ema_updates()`` from the host integers of ``host_cut()`` and the device count of skipped steps read elsewhere"""
        e = cut['ema']
        if e['decay'] is None:
            return e['done']
        return e['done'] + e['calls'] - max(0, cut['skipped_folded'] + (skipped if cut['guard_flags'] is not None else 0) - e['skip_base'])

    def _advance_ema(self):
        """one step has been issued (the eager step(), a replay: lirec_amd.graph)"""
        if self._ema_decay is not None:
            self._ema_calls += 1

    def _ema_not_recording(self, what):
        if ops.CommandList.mark() >= 0:
            raise RuntimeError('FusedAdam.%s: not while a step is being recorded (a command list holds launches, not this copy)' % what)

    @torch.no_grad()
    def ema_reset(self):
        """shadow <- parameters, count <- 0 (``AveragedModel``'s first update is this copy)"""
        self._ema_not_recording('ema_reset()')
        self._ensure_state()
        self._ensure_ema(self.model.flat_params(), force=True)
        self._join_side()
        self._ema.copy_(self.model.flat_params())
        self._ema_done, self._ema_calls, self._ema_skip_base = 0, 0, self.skipped_total()

    def _ema_stale(self):
        sync = getattr(self.model, 'grad_sync', None)
        return sync is not None and sync.sharded and sync.real_world > 1 and getattr(self, '_consolidated_at', None) != self._step

    def ema_state_dict(self):
        """name -> tensor, shaped like ``model.state_dict()``: the averaged parameters as views of the shadow (buffers, if the model
        has any, as the model holds them).  Loads into a fresh model with ``load_state_dict``."""
        self._ensure_state()
        self._ensure_ema(self.model.flat_params(), force=True)
        sd = self.model.state_dict()             # (joins the side stream: its lerp may still be running behind a replayed step)
        if self._ema_stale():
            import warnings
            warnings.warn('FusedAdam.ema_state_dict(): sharded data-parallel update -- the shadow outside this rank\'s slices is stale; '
                          'call optimizer.consolidate_state() on EVERY rank first (a collective)', RuntimeWarning, stacklevel=2)
        return self.ema_state_dict_from(self._ema, sd, self.model._offsets)

    @staticmethod
    def ema_state_dict_from(ema, sd, offsets):
        """``ema_state_dict()`` over the flat shadow ``ema`` (the optimiser's, or a host copy of it), a ``model.state_dict()``
        ``sd`` that names the entries and gives the shapes (and the values of what is no parameter) and the model's ``_offsets``"""
        from collections import OrderedDict
        out = OrderedDict()
        for k, v in sd.items():
            if k in offsets:
                off, n = offsets[k]
                out[k] = ema[off:off + n].view(v.shape)
            else:
                out[k] = v
        return out

    @torch.no_grad()
    def load_ema_state_dict(self, sd, updates=None):
        """the shadow from ``sd`` (every parameter of the model must be in it, with its shape); ``updates``: the count to go on from"""
        self._ema_not_recording('load_ema_state_dict()')
        self._ensure_state()
        self._ensure_ema(self.model.flat_params(), force=True)
        missing = [n for n in self.model._offsets if n not in sd]
        if missing:
            raise KeyError('FusedAdam.load_ema_state_dict: missing %s' % ', '.join(missing))
        self._join_side()
        for n, (off, k) in self.model._offsets.items():
            t = torch.as_tensor(sd[n])
            if t.numel() != k:
                raise ValueError('FusedAdam.load_ema_state_dict: %s has %d elements, the model\'s has %d' % (n, t.numel(), k))
            self._ema[off:off + k].copy_(t.reshape(-1))
        if updates is not None:
            self._ema_done, self._ema_calls, self._ema_skip_base = int(updates), 0, self.skipped_total()

    @contextlib.contextmanager
    def ema_weights(self):
        """``with optimizer.ema_weights():`` -- the model computes with the averaged weights inside (an evaluation, a checkpoint of
        ``model.state_dict()``), and gets its training weights back, bit for bit, on the way out.  By VALUE, through a temporary
        copy: a recorded step holds the buffers' addresses.  In front of both directions what ``Model.load_state_dict`` does before
        values change: the side stream joined, the q32b shadow of the first-layer weights and the gate's staged weights stale."""
        self._ema_not_recording('ema_weights()')
        self._ensure_state()
        flat = self.model.flat_params()
        self._ensure_ema(flat, force=True)
        if self._ema_stale():
            import warnings
            warnings.warn('FusedAdam.ema_weights(): sharded data-parallel update -- the shadow outside this rank\'s slices is stale; '
                          'call optimizer.consolidate_state() on EVERY rank first (a collective)', RuntimeWarning, stacklevel=3)

        def about_to_write():
            self._join_side()
            self.model._w1q_valid = False
            if self.lanes is not None:
                self.lanes.params_written()
        with torch.no_grad():
            about_to_write()
            backup = flat.clone()
            flat.copy_(self._ema)
        try:
            yield self
        finally:
            with torch.no_grad():
                about_to_write()
                flat.copy_(backup)

    def _join_side(self):
        if self.lanes is not None:
            self.lanes.join()

    def _lerp(self, flat, a, b):
        """the average of stretch [a, b) follows the stretch's update, on the stream current here; guarded on the guarded route"""
        if self._ema_w is not None and b > a:
            ops.ema_step(self._ema[a:b], flat[a:b], self._ema_w, guard=self._clip_out if self._guard_now else None)

    # -- parameter groups -------------------------------------------------------
    def resolve_device_hyper(self):
        """A decoupled group needs the table route (the by-value launches have no such form).  Called by the constructor,
        ``hyper_rows()``, ``step()``, ``load_state_dict()`` and the recorded step's key: with ``device_hyper`` left to default in the
        constructor it is switched on from here on (a step recorded by value then refuses to replay: its key changed); with an
        explicit ``device_hyper=False`` this raises.  Returns ``device_hyper``."""
        if not self.device_hyper and any(g.get('decoupled_weight_decay') for g in self.param_groups):
            if self._device_hyper_arg is not None:
                raise ValueError('FusedAdam: a group with decoupled_weight_decay needs device_hyper (the by-value launches know '
                                 'coupled weight decay only), and device_hyper=False was asked for')
            self.device_hyper = True
            self._ranges_key = None
        return self.device_hyper

    def _resolve_groups(self, param_groups, params):
        """the constructor's ``param_groups`` with names replaced by the parameter objects; every parameter of the model in
        exactly one group, at most MAX_GROUPS groups"""
        if isinstance(param_groups, dict) or not isinstance(param_groups, (list, tuple)) or not param_groups:
            raise ValueError('FusedAdam: param_groups must be a non-empty list of dicts')
        if len(param_groups) > self.MAX_GROUPS:
            raise ValueError('FusedAdam: %d parameter groups, at most %d' % (len(param_groups), self.MAX_GROUPS))
        by_name = dict(zip(self._names, params))
        seen, out = {}, []
        for i, grp in enumerate(param_groups):
            if not isinstance(grp, dict) or 'params' not in grp:
                raise ValueError('FusedAdam: parameter group %d is not a dict with \'params\'' % i)
            members = grp['params']
            members = [members] if isinstance(members, (str, torch.Tensor)) else list(members)
            ps = []
            for x in members:
                if isinstance(x, str):
                    if x not in by_name:
                        raise ValueError('FusedAdam: parameter group %d names %r, which is no parameter of the model' % (i, x))
                    x = by_name[x]
                if not any(x is p for p in params):
                    raise ValueError('FusedAdam: parameter group %d holds a tensor that is no parameter of the model' % i)
                if id(x) in seen:
                    raise ValueError('FusedAdam: a parameter is in parameter groups %d and %d' % (seen[id(x)], i))
                seen[id(x)] = i
                ps.append(x)
            out.append(dict(grp, params=ps))
        missing = [n for n, p in zip(self._names, params) if id(p) not in seen]
        if missing:
            raise ValueError('FusedAdam: parameters in no parameter group: %s' % ', '.join(missing))
        return out

    def add_param_group(self, param_group):
        if getattr(self, '_layout_fixed', False):
            raise RuntimeError('FusedAdam.add_param_group: the groups are fixed at construction (the flat parameter layout is); '
                               'pass param_groups= to the constructor')
        super().add_param_group(param_group)

    def group_membership(self):
        """the group index of every parameter, in ``model.named_parameters()`` order"""
        return tuple(self._group_of[n] for n in self._names)

    def group_names(self):
        """the parameter names of every group, in the groups' own order (the numbering of ``state_dict()``)"""
        name_of = {id(p): n for n, p in zip(self._names, self.model._plist)}
        return [[name_of[id(p)] for p in grp['params']] for grp in self.param_groups]

    def hyper_rows(self):
        """(lr, beta1, beta2, eps, weight_decay, decoupled) of every group as ``param_groups`` has them now, checked as at
        construction (a decoupled group with ``device_hyper=False``: ValueError)"""
        self.resolve_device_hyper()
        rows = []
        for grp in self.param_groups:
            lr, betas, eps, wd = float(grp['lr']), (float(grp['betas'][0]), float(grp['betas'][1])), float(grp['eps']), float(grp['weight_decay'])
            self._check_values(lr, betas, eps, wd)
            rows.append((lr, betas[0], betas[1], eps, wd, bool(grp.get('decoupled_weight_decay', False))))
        return tuple(rows)

    def _issuing_streams(self):
        """the streams that issue Adam launches, as {role: raw handle or None (= the current one)}"""
        m = self.model
        roles = {'main': None}
        # (the side stream only where step() can put an update on it: no lane made, no table written, for a run that never does)
        lane = None
        if self.lanes is not None and m.flat_params().is_cuda and getattr(opt, 'adam_on_side_stream', True) \
                and getattr(getattr(m, 'grad_sync', None), 'world', 1) <= 1:
            lane = self.lanes.wgrad(m.flat_params().device)
        if lane is not None:
            roles['side'] = lane.handle
        early = getattr(getattr(m, 'grad_sync', None), '_launch_stream', None)
        if early is not None:
            roles['early'] = C.c_void_p(early.cuda_stream)
        return roles

    def sync_hyper(self, main=None):
        """Under ``device_hyper``: compare ``param_groups`` with what the table of each issuing stream last received and send what
        differs -- one lirec_adam_hyper_write per stale table, ON THE STREAM THAT READS IT (``main``: the raw handle of the stream
        the caller's Adam launches go to, None = the current one); nothing otherwise.  Returns the number of writes issued.
        Never inside a recording: a command list holds the tables' addresses, not their values."""
        if not self.resolve_device_hyper():
            return 0
        rows = self.hyper_rows()
        stale = [(role, h) for role, h in self._issuing_streams().items() if self._tables.get(role, (None, None))[1] != rows]
        if not stale:
            return 0
        if ops.CommandList.mark() >= 0:
            raise RuntimeError('FusedAdam: the hyper-parameter tables are not current while a step is being recorded (a command '
                               'list never contains a write to them); call sync_hyper() before the recording begins')
        dev = self.model.flat_params().device
        for role, h in stale:
            if role not in self._tables:
                # (torch.empty: no fill launch on the current stream that could meet the write on another one)
                self._tables[role] = [torch.empty(8 * self.MAX_GROUPS, dtype=torch.float32, device=dev), None]
            if role == 'main' and main is not None:
                h = main
            if h is None:
                ops.adam_hyper_write(self._tables[role][0], rows)
            else:
                with ops.on_stream(h):
                    ops.adam_hyper_write(self._tables[role][0], rows)
            self._tables[role][1] = rows
        return len(stale)

    def _table(self, role):
        """the table of issuing stream ``role``, which must be current (sync_hyper)"""
        t = self._tables.get(role)
        if t is None or t[1] != self._rows_now:
            raise RuntimeError('FusedAdam: the hyper-parameter table of the %s stream is not current (sync_hyper() was not called '
                               'for it, or param_groups changed inside a step)' % role)
        return t[0]

    # -- flat state -----------------------------------------------------------
    def _ensure_state(self):
        flat = self.model.flat_params()
        if self._m is None or self._m.device != flat.device or self._m.numel() != flat.numel():
            old = {id(p): self.state.get(p) for p in self.model.parameters()}
            self._m = torch.zeros_like(flat)
            self._v = torch.zeros_like(flat)
            if self.lanes is not None:
                self.lanes.side_ticket = torch.zeros(1, dtype=torch.int32, device=flat.device)      # (lirec_adam_step_counted's arrival counter)
            if self._guard_flags is not None:
                self._fold_skipped()   # (the count of skipped steps does not outlive its buffer)
            self._clip_out = None
            pd = dict(self.model.named_parameters())
            for n, (off, k) in self.model._offsets.items():
                p = pd[n]
                m = self._m[off:off + k].view(p.shape)
                v = self._v[off:off + k].view(p.shape)
                st = old.get(id(p))
                if st:
                    m.copy_(st['exp_avg']); v.copy_(st['exp_avg_sq'])
                self.state[p] = {'step': torch.tensor(float(self._step - self._lag.get(n, 0))), 'exp_avg': m, 'exp_avg_sq': v}
            if flat.is_cuda:
                # (the fills above are on the current stream; the first bucket's update runs on ANOTHER stream -- the weight-gradient
                #  side stream, or the collectives' launch stream -- that was ordered behind this one during backward, i.e. before
                #  these fills were enqueued: without this one-time wait the very first step could read the moments unzeroed.
                #  Seen as NaN parameters in one of ~5 runs of the two-rank test, where two processes share the GPU.)
                torch.cuda.current_stream(flat.device).synchronize()
        self._ensure_ema(flat)

    def zero_grad(self, set_to_none: bool = False, counters=None, zero: bool = True):
        """One memset over the flat gradient buffer (gradient views stay attached).  ``counters`` = (int64 device tensor,
        increments): advanced by the same launch (lirec_amd.graph: the step counters of a replayed step).  ``zero=False``
        (lirec_amd.graph only): the counters alone -- the step's weight gradients overwrite the buffer (ops.set_grad_overwrite)."""
        g = self.model._flat_grad
        self._hold_sync()
        if self._accum_k > 1 and self._accum_phase != 0 and counters is None:
            return                     # (inside a window: the micro-batches taken so far stay; p.grad is their unscaled sum)
        if counters is not None and not zero:
            ops.counter_add(counters[0], counters[1])
            return
        if counters is not None:
            if g is not None and g.is_cuda and (g.data_ptr() & 15) == 0:
                ops.zero_count(g, counters[0], counters[1])
                if set_to_none:
                    for p in self.model.parameters():
                        p.grad = None
                return
            ops.counter_add(counters[0], counters[1])
        if g is not None and not g.is_cuda:
            g.zero_()
        elif g is not None:
            ops.zero_(g)
        if set_to_none:
            for p in self.model.parameters():
                p.grad = None

    # -- gradient clipping ------------------------------------------------------
    def _clip_max(self):
        """the bound of the global-norm clip as the kernels get it, or None when clipping is off (``max_grad_norm`` None or 0)"""
        c = self.max_grad_norm
        if c is None or c == 0:
            return None
        c = float(c)
        if not c > 0.0:
            raise ValueError('FusedAdam.max_grad_norm must be positive (or None / 0 for no clipping), not %r' % (self.max_grad_norm,))
        return c

    def _clip_buffers(self):
        if self._clip_out is None or self._clip_out.device != self.model.flat_params().device:
            from ._lib import CLIP_PARTIALS
            dev = self.model.flat_params().device
            self._clip_out = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
            self._skipped_dev = torch.zeros(1, dtype=torch.int64, device=dev)
            self._clip_sq = torch.zeros(1, dtype=torch.float64, device=dev)
            self._clip_partials = torch.zeros(CLIP_PARTIALS, dtype=torch.float64, device=dev)
        return self._clip_out

    @property
    def clip_coef(self):
        """0-d device tensor (a view: no synchronisation): the coefficient the last step multiplied its gradients by --
        min(1, max_grad_norm / (grad_norm + 1e-6)); 1 before the first clipped step"""
        return self._clip_buffers()[0]

    @property
    def grad_norm(self):
        """0-d device tensor (a view: no synchronisation): the L2 norm of the last clipped step's gradient over the trainable
        parameters AS THE UPDATE SAW IT (times ``grad_scale``), before clipping -- what ``clip_grad_norm_`` returns"""
        return self._clip_buffers()[1]

    @property
    def found_nonfinite(self):
        """0-d device float (a view: no synchronisation): 1.0 when the last guarded step (``skip_nonfinite``) found a NaN or an Inf
        in the trainable gradients and was skipped, else 0"""
        return self._clip_buffers()[2]

    @property
    def skipped_steps(self):
        """0-d device int64 (a view: no synchronisation): the guarded steps skipped since the optimiser last folded them into its
        step (a change of the frozen set, the guard switched off, ``load_state_dict``) -- in a run without those, all of them"""
        self._clip_buffers()
        return self._skipped_dev[0]

    # -- skipped steps: the accounting ---------------------------------------------
    @staticmethod
    def updates_received(step, lags, flags, skipped):
        """per-parameter number of updates, torch.optim.Adam's ``state[p]['step']``: ``step`` calls so far, ``lags`` and ``flags``
        (requires_grad during the interval ``skipped`` was counted in) in parameter order.  A trainable parameter sat the skipped
        steps out; a frozen one's lag has grown with every call, skipped or not."""
        return [step - lag - (skipped if f else 0) for lag, f in zip(lags, flags)]

    @staticmethod
    def folded(step, lags, flags, skipped):
        """(step, lags) after a fold of ``skipped`` steps: the step loses them, and so does the lag of every parameter frozen
        throughout -- ``updates_received`` with 0 skipped gives the same counts as before"""
        return step - skipped, [lag if f else lag - skipped for lag, f in zip(lags, flags)]

    def _read_skipped(self):
        return int(self._skipped_dev.item()) if self._guard_flags is not None and self._skipped_dev is not None else 0

    def _fold_skipped(self):
        """S into ``_step`` and the frozen parameters' lags; the device count back to 0.  Only where the step is by value."""
        if self._step_dev is not None:
            raise RuntimeError('FusedAdam: the frozen set changed, or skip_nonfinite was switched off, while a recorded step holds the '
                               'step on the device -- the skipped steps cannot be folded in there; release() the recorded step first')
        S = self._read_skipped()
        if S:
            self._step, lags = self.folded(self._step, [self._lag.get(n, 0) for n in self._names], self._guard_flags, S)
            self._lag = {n: lag for n, lag in zip(self._names, lags) if lag}
            self._ranges_key = None
            self._skipped_dev.zero_()
            self._skipped_folded += S
        self._guard_flags = None

    def skipped_total(self):
        """every step skipped so far, folded ones included, as a host int (one read of the device count: synchronises)"""
        return self._skipped_folded + self._read_skipped()

    def continue_skipped_from(self, total):
        """``skipped_total()`` goes on from ``total`` (a resumed run: ``load_state_dict`` has the per-parameter steps, in which the
        skipped ones are already missing, and starts the count at 0).  Nothing the update reads changes; the average's count of
        its own updates, which takes the skipped steps off, keeps its value."""
        delta = int(total) - self.skipped_total()
        self._skipped_folded += delta
        self._ema_skip_base += delta

    def fold_if_due(self):
        """at the top of an eager step, and before a recording attaches its counters: fold when the frozen set is no longer the one
        the skipped steps were counted under, or the guard is off"""
        if self._guard_flags is not None and (not self.skip_nonfinite or self._flags() != self._guard_flags):
            self._fold_skipped()

    def _finalize(self, partials, mode, count=False):
        """the finalize of the route: the guard's (bound 0 = no clipping) with the guard on, the clip's otherwise"""
        if self._guard_now:
            ops.clip_finalize_guard(partials, self._clip_sq, mode, self._scale(), self._clip_now or 0.0, self._clip_out,
                                    self._skipped_dev, count)
        else:
            ops.clip_finalize(partials, self._clip_sq, mode, self._scale(), self._clip_now, self._clip_out)

    def _scaled(self):
        """the context the route's Adam launches are issued in"""
        if self._guard_now:
            return ops.adam_guard(self._clip_out, self._skipped_dev)
        return ops.adam_clip(self._clip_out[0:1])

    def _clip_accumulate(self, gbuf, ranges, first):
        """sum of squares of ``gbuf`` over ``ranges`` = [(offset, length)] into the device double (the first table of a step sets
        it, the others add) and the coefficient of the sum so far; returns ``first`` for the next call"""
        for ch in self._chunks([r for r in ranges if r[1] > 0]):
            ops.grad_sq_partials(gbuf, ch, self._clip_partials)
            self._finalize(self._clip_partials, 0 if first else 1)
            first = False
        return first

    # -- per-parameter statistics ---------------------------------------------------
    @staticmethod
    def stat_factors(t, beta1, beta2):
        """(inv_bc1, inv_sqrt_bc2) of update ``t`` >= 1 as a lirec_param_stat_entry carries them: 1 / (1 - beta1^t) and
        1 / sqrt(1 - beta2^t), computed in double and rounded to fp32"""
        t = max(int(t), 1)
        return (C.c_float(1.0 / (1.0 - float(beta1) ** t)).value, C.c_float(1.0 / (1.0 - float(beta2) ** t) ** 0.5).value)

    def _stats_refusals(self, what):
        self._ema_not_recording(what)
        if getattr(getattr(self.model, 'grad_sync', None), 'world', 1) > 1:
            from ._lib import LirecError
            raise LirecError('FusedAdam.%s: single-process only -- under data parallelism the moments are current in this rank\'s '
                             'slices alone and the reduced gradient lives in slice buffers, so a defined answer needs collectives, '
                             'which this call deliberately does not issue' % what)

    @torch.no_grad()
    def param_stats(self, update=True):
        """Per-parameter statistics of the gradient, the weight and the last Adam step, computed on the device in one
        deterministic pass over the flat buffers (lirec_param_stats: two launches per 64 parameters, the same bits every time).
        Returns a ``ParamStats``: ``names``, the device ``table`` (no synchronisation) and ``host()`` -- one copy, then
        {name: ParamStat}.  One row per parameter, over exactly its ``numel`` elements: the alignment gaps of the flat layout are in
        no row.

        Gradient columns, for the parameters that require grad NOW: ``grad_norm`` = the L2 norm of the gradient buffer times
        ``grad_scale`` -- over k inside or at the end of an accumulation window, where the buffer holds the unscaled sum so far --,
        i.e. AS THE UPDATE SEES IT; ``grad_absmax`` scaled the same way; ``grad_nonfinite`` the count of NaN / Inf elements, which
        enter neither of the two.  With clipping on and no non-finite value, the root of the sum of the trainable parameters'
        squared norms is ``optimizer.grad_norm``.
        Parameter columns, for every parameter: ``param_norm``, ``param_absmax``, ``param_nonfinite``.
        Update columns (``update=True``), for the parameters that have received at least one update: with t that number of
        updates and lr, betas, eps of the parameter's group, u = (m / (1 - beta1^t)) / (sqrt(v) / sqrt(1 - beta2^t) + eps) and
        ``update_norm`` = lr ||u||, ``update_absmax`` = lr max|u|, ``update_ratio`` = update_norm / param_norm (None where the
        norm is 0).  This is the size of the last APPLIED Adam step as the moments hold it now: decoupled weight decay's separate
        term p (1 - lr wd) is not in it, and where the last ``step()`` was a hold or was skipped it still describes the step
        before.  t comes from ``updates_received`` -- lags, and the device count of skipped steps when a guard has been on: that
        is ONE READ OF A DEVICE INT, A SYNCHRONISATION, as ``skipped_total()`` is; ``update=False`` never synchronises.
        A column that was not asked for -- gradient and update columns of a frozen parameter, update columns of a parameter never
        updated or with ``update=False`` -- is None in ``host()``.

        Joins the side stream first, so it is correct between replays of a recorded step.  RuntimeError while a step is being
        recorded; LirecError under data parallelism (see the message)."""
        from ._lib import PARAM_STATS_COLS, PARAM_STATS_MAX_RANGES, STAT_GRAD, STAT_PARAM, STAT_UPDATE
        self._stats_refusals('param_stats()')
        self._ensure_state()
        self._join_side()
        m = self.model
        flat, g = m.flat_params(), m.flat_grads(attach=True)
        live = self._flags()
        counts = [0] * len(self._names)
        if update:
            S = self._read_skipped()
            counts = self.updates_received(self._step, [self._lag.get(n, 0) for n in self._names],
                                           self._guard_flags if S else live, S)
        entries, flags, lrs = [], [], []
        for n, f, t in zip(self._names, live, counts):
            off, k = m._offsets[n]
            grp = self.param_groups[self._group_of[n]]
            fl = STAT_PARAM | (STAT_GRAD if f else 0) | (STAT_UPDATE if t >= 1 else 0)
            fac = self.stat_factors(t, *grp['betas']) + (float(grp['eps']),) if t >= 1 else (1.0, 1.0, 0.0)
            entries.append((off, k, fl) + fac)
            flags.append(fl)
            lrs.append(float(grp['lr']))
        table = torch.empty((len(entries), PARAM_STATS_COLS), dtype=torch.float64, device=flat.device)
        ws = getattr(self, '_stats_ws', None)
        if ws is None or ws.device != flat.device:
            ws = self._stats_ws = torch.empty(ops.param_stats_ws_bytes(PARAM_STATS_MAX_RANGES) // 8, dtype=torch.float64, device=flat.device)
        row = 0
        for ch in self._chunks(entries, PARAM_STATS_MAX_RANGES):      # (one stream: a chunk's launches are through with ws before the next's)
            ops.param_stats(flat, g, self._m, self._v, ch, table[row:row + len(ch)], ws)
            row += len(ch)
        return ParamStats(self._names, table, flags, self._scale(), lrs)

    def nonfinite_params(self):
        """the names of the parameters whose gradient holds a NaN or an Inf right now: one ``param_stats(update=False)`` and one
        read.  After a step that ``skip_nonfinite`` skipped it names the culprits -- the gradients stay as backward left them.
        The refusals of ``param_stats()``."""
        self._stats_refusals('nonfinite_params()')
        return [n for n, s in self.param_stats(update=False).host().items() if s.grad_nonfinite]

    # -- the update's route ----------------------------------------------------------
    def route(self, pipelined=False):
        """The ``Route`` the next ``step()`` takes -- EVERY exclusion between the features is written here and nowhere else (DESIGN
        4.4, "The update's route").  ``pipelined``: for a recording in the input-pipeline form.  No device read, no allocation."""
        m, k, sync = self.model, self._accum_k, getattr(self.model, 'grad_sync', None)
        parallel = sync is not None and sync.world > 1
        window = k > 1 and self._win_dev is not None
        # (skip_nonfinite: the norm route whether or not a bound is set -- the decision needs the finished gradients as the norm does)
        guard = bool(self.skip_nonfinite)
        norm = guard or bool(self.max_grad_norm)
        refuse = None
        if k > 1 and pipelined:
            refuse = ('RecordedTrainStep(next_batch=...): the input-pipeline form is not built with gradient accumulation '
                      '(accumulate_steps = %d) -- record the plain form' % k)
        elif k > 1 and parallel:
            refuse = ('RecordedTrainStep: gradient accumulation under data parallelism is not recorded (the bucket reductions '
                      'are issued from the host, which a replay gives no hold / apply decision) -- run the eager step')
        elif k > 1 and norm:
            refuse = ('RecordedTrainStep: gradient accumulation with max_grad_norm / skip_nonfinite is not recorded (the norm '
                      'launches and the finalize have no hold gate) -- run the eager step')
        elif norm and parallel:
            refuse = ('RecordedTrainStep: gradient clipping / skip_nonfinite under data parallelism is not recorded (the all-reduce '
                      'of the squared norm sits between the recorded launches) -- run the eager step')
        # The folded first-layer update: single GPU; not on the norm route (the norm needs the finished first-layer gradients: they
        # are updated with the rest, clipped); not accumulating (the fold has no hold gate: it would update on every micro-batch)
        first = 'ordinary'
        if sync is None and self.lanes is not None and hasattr(m, 'first_layer_range') and not norm and k == 1:
            first = self._first_layers()
        # lane 0 and the deferred join: the norm needs EVERY gradient finished, so nothing is updated beside the tail of backward; the
        # window's update is issued whole on the caller's stream under the hold gate (lane 0's counter: begin_micro_step)
        return Route(hold=k > 1 and not window and not self.window_after(self._accum_phase, k)[1], norm=norm, guard=guard,
                     window=window, parallel=parallel, lane0=self.lanes is not None and not (norm or window or parallel), first=first,
                     may_overwrite=k == 1, refuse=refuse)

    def _first_layers(self):
        """``Route.first`` as the frozen set and the groups allow it (cached with the trainable ranges)"""
        self.resolve_device_hyper()
        self.trainable_ranges()            # (refreshes the key: flags, lags, layout, device_hyper)
        if self._first is None or self._first[0] is not self._ranges_key:
            # (the folded launch updates EVERY first-layer parameter with the one global step: first_layer_fold_ranges -- by value
            #  that is the one range of the whole bucket; under ``device_hyper`` one group, one row, or several, the map)
            fold = self.first_layer_fold_ranges()
            if fold is not None:
                kind = 'value' if not self.device_hyper else 'row' if len(fold) == 1 else 'map'
            else:
                kind = 'ordinary' if self.trainable_ranges(*self.model.first_layer_range()[:2]) else 'untouched'
            self._first = (self._ranges_key, kind)
        return self._first[1]

    def arm_first_layer_update(self):
        """For a caller that issues backward and step as a unit (lirec_amd.graph.RecordedTrainStep; single GPU): the NEXT backward
        folds the update of the first layers of both embeddings (the last gradient bucket, 10 M parameters at the bench shape)
        into the stream-K reduce that finishes their weight gradient (lirec_fused_adam, include/lirec_hip.h).  That launch also
        keeps the q32b form of the new weights current (model.refresh_w1q), so the next forward stages no first-layer weights --
        and the step() that follows leaves that range alone.  One shot; a backward that cannot take it (another kernel path)
        ignores it and step() updates the range as usual."""
        self._ensure_state()
        m = self.model
        if self._step_dev is None:
            self.fold_if_due()
        first = self.route().first
        if first not in ('value', 'row', 'map'):
            return False
        row = hmap = None
        if first != 'value':
            # (the row -- the rows -- of the table of the stream that runs the backward's tail)
            rs = self.first_layer_fold_ranges()
            self.sync_hyper()
            self._rows_now = self.hyper_rows()
            if first == 'row':
                row = self._table('main')[8 * rs[0][3]:8 * rs[0][3] + 8]
            else:
                hmap = (self._table('main'), [(a, b - a, grp) for a, b, _, grp in rs])
        grp = self.param_groups[0]
        flat, g = m.flat_params(), m.flat_grads(attach=True)
        hyper = (max(self._step + (1 if self._step_dev is None else 0), 1), grp['lr'], grp['betas'][0], grp['betas'][1], grp['eps'],
                 grp['weight_decay'], self.grad_scale, self._step_dev)
        lo, hi, n_params = m.first_layer_range()
        valid = bool(getattr(m, '_w1q_valid', False)) and getattr(m, '_w1q_mode', None) == ops.get_gemm_mode()
        # (with ``row`` the five values above are ignored: lirec_set_adam_hyper_row; with ``hmap`` each parameter reads the row of its
        #  group: lirec_set_adam_hyper_map)
        self.lanes.fold = (ops.fused_adam_args(flat, g, self._m, self._v, n_params, *hyper, wq=m._w1q_buf if valid else None,
                                               wq_first=m._w1q_first if valid else 0), row, hmap)
        return True

    def first_layer_fold_ranges(self):
        """The ranges (start, end, 0[, group]) of the first-layer bucket when the folded update can take it -- every first-layer
        parameter trainable with lag 0, in at most 16 ranges (under ``device_hyper`` one range: one group; by value: one) -- or None"""
        from ._lib import ADAM_MAP_MAX
        m = self.model
        lo, hi, _ = m.first_layer_range()
        rs = self.trainable_ranges(lo, hi)
        inside = [n for n, (off, k) in m._offsets.items() if lo <= off < hi]
        flags = dict(zip(self._names, self._flags()))
        if not rs or len(rs) > ADAM_MAP_MAX or any(r[2] != 0 for r in rs) or not all(flags[n] for n in inside):
            return None
        return rs

    # -- frozen parameters ------------------------------------------------------
    def _flags(self):
        return tuple(p.requires_grad for p in self.model._plist)

    def all_trainable(self):
        """every parameter requires grad and has received every update (the state this optimiser was written for)"""
        return not self._lag and all(self._flags())

    def frozen_key(self):
        """what a recorded step has baked in of the frozen set: the requires_grad flags and the trainable parameters' lags
        (lirec_amd.graph.RecordedTrainStep.hyper_key); () with nothing frozen and no lag"""
        if self.all_trainable():
            return ()
        flags = self._flags()
        return (flags, tuple(self._lag.get(n, 0) for n, f in zip(self._names, flags) if f))

    @staticmethod
    def merged_ranges(offsets, trainable, lags, extent, groups=None):
        """The trainable ranges [(start, end, lag)] of a flat layout, ascending -- with ``groups`` (name -> group index; parameter
        groups): [(start, end, lag, group)], and neighbours merge only when lag AND group are the same.  ``offsets``: name -> (offset, numel) in flat
        order; ``trainable``: name -> bool; ``lags``: name -> int (missing = 0); ``extent``: the buffer's length.  Neighbours in the
        layout that are both trainable with the same lag are merged ACROSS the alignment gap between them (the gap holds zeros in
        all four buffers, which the update leaves zeros -- as the whole-buffer launch always has), and a trainable last parameter
        takes the buffer's tail: with everything trainable the result is the one range (0, extent, 0)."""
        out, prev_live = [], False
        names = list(offsets)
        for i, n in enumerate(names):
            off, k = offsets[n]
            live = bool(trainable[n])
            if live:
                end = extent if i == len(names) - 1 else off + k
                lag = int(lags.get(n, 0))
                tail = (lag,) if groups is None else (lag, int(groups[n]))
                if prev_live and out[-1][2:] == tail:
                    out[-1] = (out[-1][0], end) + tail
                else:
                    out.append((off, end) + tail)
            prev_live = live
        return out

    def trainable_ranges(self, lo=None, hi=None):
        """merged_ranges of the model as it is now (cached on the flags and lags), cut to [lo, hi) when given; under
        ``device_hyper`` with each range's group: (start, end, lag, group)"""
        m = self.model
        flags = self._flags()
        key = (flags, tuple(sorted(self._lag.items())), id(m._offsets), bool(self.device_hyper))
        if key != self._ranges_key:
            self._ranges = self.merged_ranges(m._offsets, dict(zip(self._names, flags)), self._lag, m._flat.numel(),
                                              self._group_of if self.device_hyper else None)
            self._ranges_key = key
        if lo is None:
            return list(self._ranges)
        return [(max(r[0], lo), min(r[1], hi)) + r[2:] for r in self._ranges if min(r[1], hi) > max(r[0], lo)]

    @staticmethod
    def _chunks(rs, most=64):
        """a list of ranges cut into the tables of single lirec_adam_step_ranges calls (64 entries at the most)"""
        return [rs[i:i + most] for i in range(0, len(rs), most)]

    def _advance_lags(self):
        """one update has been issued: every parameter that sat it out falls one further behind"""
        if self._lag or not all(self._flags()):
            for n, f in zip(self._names, self._flags()):
                if not f:
                    self._lag[n] = self._lag.get(n, 0) + 1

    def _update(self, flat, g, a, b, args, **kw):
        """``_adam`` of stretch [a, b), then the stretch's share of the weight average (``ema_decay``) directly behind it on the
        same stream -- also where nothing in the stretch is trainable and no Adam launch was issued.  Returns ``_adam``'s count."""
        n = self._adam(flat, g, a, b, args, **kw)
        self._lerp(flat, a, b)
        return n

    def _adam(self, flat, g, a, b, args, g_is_slice=False, counted=None, last=True, role='main'):
        """The update of stretch [a, b) of the flat buffers -- ``g``: the flat gradient buffer, or (``g_is_slice``) the b - a
        gradients of the stretch on their own.  One zero-lag range: the whole-stretch launch, as ever; nothing trainable: no
        launch; anything else: lirec_adam_step_ranges, 64 ranges a call.  ``counted`` = (count_dev, ticket): the step from the
        side stream's own counter, ``last``: this stretch is the last of the update (the last launch advances the counter).
        Under ``device_hyper`` every stretch is lirec_adam_step_groups launches, reading the table of issuing stream ``role``.
        Returns the number of launches issued."""
        bufs = (flat[a:b], g if g_is_slice else g[a:b], self._m[a:b], self._v[a:b])
        step, hyper, gscale, step_dev = args[0], args[1:6], args[6], args[7]
        if counted is not None:
            step = 0
        # the launch form: the groups' table, the whole stretch, or its trainable ranges
        if self.device_hyper:
            form, rs = 'groups', self.trainable_ranges(a, b)
            table, n_groups = self._table(role), len(self.param_groups)
        else:
            rs = [(a, b, 0)] if self._all_live else self.trainable_ranges(a, b)
            form = 'whole' if rs == [(a, b, 0)] else 'ranges'
        chunks = self._chunks(rs)
        for i, ch in enumerate(chunks):
            rel = [(r[0] - a, r[1] - r[0]) + tuple(r[2:]) for r in ch]
            # where the step comes from: the side stream's counter, which the update's last launch advances, or step / step_dev
            if counted is not None:
                src = dict(count_dev=counted[0], ticket=counted[1], advance=last and i == len(chunks) - 1)
            else:
                src = dict(step_dev=step_dev)
            if form == 'groups':
                ops.adam_step_groups(*bufs, rel, table, n_groups, step, gscale, **src)
            elif form == 'ranges':
                ops.adam_step_ranges(*bufs, rel, step, *hyper, gscale, **src)
            elif counted is not None:
                ops.adam_step_counted(*bufs, *hyper, gscale, **src)
            else:
                ops.adam_step(*bufs, step, *hyper, gscale, **src)
        return len(chunks)

    @staticmethod
    def _minus(lo, hi, skip):
        """[lo, hi) without the ranges in ``skip``: a list of (a, b); a range with b <= a is empty"""
        out, a = [], lo
        for s0, s1 in sorted(skip):
            if s1 <= s0 or s1 <= a or s0 >= hi:
                continue
            if s0 > a:
                out.append((a, min(s0, hi)))
            a = max(a, s1)
        if a < hi:
            out.append((a, hi))
        return [(x, y) for x, y in out if y > x]

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._ensure_state()
        route = self.route()
        if route.hold:
            # Gradient accumulation, eager: the host decides -- a hold step issues nothing (no reduction under data parallelism
            # either: GradSync.hold) and only moves the phase.  (Recorded, ``route.window``: every micro-step issues the whole
            # update under the hold gate and the device decides.)
            if self.lanes is not None:
                self.lanes.after_backward = None       # (one-shot of the backward: no update takes it)
                self._join_side()
        elif route.parallel and route.norm:
            self._step_parallel_clipped(*self._begin_update(route))
        elif route.parallel:
            self._step_parallel(*self._begin_update(route))
        else:
            self._step_single(route, *self._begin_update(route))
        if route.hold or self._step_dev is None:
            # (the host mirrors, _step included: a recorded step's caller advances them itself -- RecordedTrainStep._advance_host)
            if self._advance_window():        # (applied: not a hold step)
                self._advance_lags()
                self._advance_ema()
        return loss

    def _begin_update(self, route):
        """the prologue of every update that is issued; returns (flat parameters, flat gradients, the launches' arguments)"""
        self.fold_if_due()                # (raises where a recorded step holds the step on the device)
        self._all_live = self.all_trainable()
        grp = self.param_groups[0]
        if self.resolve_device_hyper():
            # (the tables as param_groups has them now; inside a recording they must be current already -- sync_hyper raises)
            self.sync_hyper()
            self._rows_now = self.hyper_rows()
        g = self.model.flat_grads(attach=True)
        if self._step_dev is None:
            self._step += 1
        # (accumulating: 1 / k folded into the scale -- by value here, by the launches themselves under the hold gate)
        args = (max(self._step, 1), grp['lr'], grp['betas'][0], grp['betas'][1], grp['eps'], grp['weight_decay'],
                self.grad_scale if route.window else self._scale(), self._step_dev)
        flat = self.model.flat_params()
        self._clip_now, self._guard_now = self._clip_max(), route.guard
        if route.norm:
            self._clip_buffers()
        if route.guard:
            self._guard_flags = self._flags()
        if route.window and route.refuse is not None:
            from ._lib import LirecError
            raise LirecError(route.refuse)
        if route.parallel:
            sync = self.model.grad_sync
            if getattr(opt, 'strict', False) and hasattr(sync, 'check_frozen_set'):
                sync.check_frozen_set(self._flags(), self.group_membership() if len(self.param_groups) > 1 else ())
            if self.lanes is not None:
                self.lanes.bucket0_on_side = False
        return flat, g, args

    def _step_parallel(self, flat, g, args):
        # data parallel: each bucket is updated as its reduction lands, the later buckets still in flight.  Sharded
        # (the default, lirec_amd.parallel): this rank holds the summed gradients of ITS slice of the bucket only, updates
        # that slice (parameters and moments), and the slices are all-gathered back into everybody's parameter buffer
        sync, done, used = self.model.grad_sync, 0, None
        for lo, hi, early in sync.wait_each():
            a, b = sync.my_slice(lo, hi)
            if early is not None:
                # (heads + gate: reduced long before backward ends, and nothing that is still to run reads them -- updated
                #  and gathered on the collective's launch stream, beside the tail of backward: GradSync.early_stream)
                with ops.on_stream(C.c_void_p(early.cuda_stream)), torch.cuda.stream(early):
                    if b > a:
                        self._update(flat, sync.grad_slice(g, lo, hi), a, b, args, g_is_slice=True, role='early')
                    sync.gather_params(lo, hi)
                used = early
            else:
                if b > a:
                    self._update(flat, sync.grad_slice(g, lo, hi), a, b, args, g_is_slice=True)
                sync.gather_params(lo, hi)
            done += hi - lo
        assert done == flat.numel(), 'gradient buckets do not cover the parameter buffer'
        if used is not None:          # the step ends when the early bucket's update has (one event)
            ops.stream_wait(ops.current_stream_handle(), C.c_void_p(used.cuda_stream))
        sync.finish_gathers()

    def _step_single(self, route, flat, g, args):
        """the single-GPU update: bucket 0 on lane 0 where the route and the backward allow it, the rest on the caller's stream"""
        sync, lanes = self.model.grad_sync, self.lanes
        if sync is not None:
            sync.wait()
        # (the first layers' bucket was updated by the backward itself -- arm_first_layer_update -- or: an update from here
        #  does not write the q32b shadow of the first-layer weights, which is stale from now on)
        skip = []
        if lanes is not None and lanes.take_fold_applied():
            skip.append((self.model.first_layer_range()[0], flat.numel()))
            # (the backward's fold ran on this stream before step() was entered: the range's average follows it here)
            self._lerp(flat, *skip[0])
        elif getattr(self.model, '_w1q_valid', False):
            # (... unless the first layers are frozen altogether: nothing writes those weights, the shadow stays current)
            if self._all_live or self.trainable_ranges(*self.model.first_layer_range()[:2]):
                self.model.invalidate_w1q()

        def update(lo, hi, role='main'):
            for a, b in self._minus(lo, hi, skip):
                self._update(flat, g, a, b, args, role=role)
        side = lanes.take_after_backward(self.model._offsets) if lanes is not None else None
        if not route.lane0:
            side = None
        if lanes is not None:
            lanes.bucket0_on_side = side is not None
        if side is not None:
            side_h, hi0 = side
            self._bucket0_on_lane0(side_h, hi0, skip, update, flat, g, args)
            update(hi0, flat.numel())
            # (the step ends when lane 0's share has -- unless a replayed step leaves it un-joined: StepLanes.may_defer)
            if not lanes.unjoined:
                ops.stream_wait(ops.current_stream_handle(), side_h)
            return
        # (no update on lane 0 after all: whatever a backward left running there writes the gradients this update reads)
        self._join_side()
        if self._step_dev is not None and lanes is not None and lanes.step_side_dev is not None and not route.window:
            ops.counter_add(lanes.step_side_dev, [1])      # (kept in step with the shared counter whichever path a step takes)
        if not route.norm:
            # (the window on the device: under the hold gate; else nothing is set)
            with ops.adam_hold(self._win_dev[1:2] if route.window else None, self._accum_k):
                update(0, flat.numel())
        else:
            # The norm is taken over the trainable ranges (frozen slices of the buffer hold whatever a shared launch left there) and
            # the whole update follows on this stream, clipped
            if skip:
                # (max_grad_norm was set between arm_first_layer_update() and this step: the backward has already applied
                #  the first layers' update, unclipped -- nothing here can take it back)
                raise RuntimeError('FusedAdam.step(): max_grad_norm / skip_nonfinite was set after the backward of this step had '
                                   'folded the first-layer update in (arm_first_layer_update); set it before the step begins')
            rs = [(0, flat.numel())] if self._all_live else [(a, b - a) for a, b, *_ in self.trainable_ranges()]
            if self._clip_accumulate(g, rs, True):
                self._clip_nothing()              # (nothing trainable: no update; norm 0, coefficient 1)
                self._lerp(flat, 0, flat.numel())
            else:
                if route.guard:   # (the one finalize of the step that counts)
                    self._finalize(None, 2, count=True)
                with self._scaled():
                    update(0, flat.numel())

    def _bucket0_on_lane0(self, side_h, hi0, skip, update, flat, g, args):
        # Single GPU with lane 0: the heads' and the gate's gradients (bucket 0, 53 % of the parameters) were finished there
        # long before the main stream is through with the layer-1 weight gradients, and the lane is ordered behind every
        # main-stream reader of these parameters.  Their update runs there, beside the MFMA-bound tail of backward.
        # (behind everything enqueued on this stream so far -- a caller may touch the gradients between backward() and step();
        #  one event, ~6 us -- unless the step is issued as a unit: the wait would also put the update behind 0.19 ms of tail)
        if not self.lanes.atomic_step:
            ops.stream_wait(side_h, ops.current_stream_handle())
        with ops.on_stream(side_h):
            if self._step_dev is None or self.lanes.step_side_dev is None:
                update(0, hi0, 'side')            # (the step by value)
                return
            # the step as THIS lane counts it ("Lanes": step_side_dev): the update launch reads the completed
            # steps (+ 1), its last workgroup advances them; stretches with nothing trainable issue no launch, the
            # counter is advanced all the same
            stretches = self._minus(0, hi0, skip)
            rs = [(a, b) for a, b in stretches if self._all_live or self.trainable_ranges(a, b)]
            if not rs:
                ops.counter_add(self.lanes.step_side_dev, [1])
            for i, (a, b) in enumerate(rs):
                self._update(flat, g, a, b, args, counted=(self.lanes.step_side_dev, self.lanes.side_ticket), last=(i == len(rs) - 1),
                             role='side')
            for a, b in stretches:            # (nothing trainable, no launch above: the average moves all the same)
                if (a, b) not in rs:
                    self._lerp(flat, a, b)

    def _clip_nothing(self):
        """a clipped step with nothing to clip: (coefficient, norm) = (1, 0), written by the finalize from a zeroed sum -- two
        tiny library launches that a command list records like the rest (the values of an earlier step must not stay)"""
        ops.zero_(self._clip_sq)
        self._finalize(None, 2)

    def _step_parallel_clipped(self, flat, g, args):
        """The data-parallel update with gradient clipping: EVERY bucket's reduction lands first (no update beside the tail of
        backward, none while later buckets are on the wire -- the coefficient needs them all); each rank squares ITS slices of the
        trainable ranges -- under the sharded update nobody holds the whole reduced gradient -- one all-reduce of the single double
        adds them up (the same bits on every rank), and the slices are updated and gathered as ever, clipped.  ``grad_scale`` =
        1 / world enters the norm: every rank gets the coefficient of the AVERAGED gradient."""
        import torch.distributed as dist
        sync, cur = self.model.grad_sync, ops.current_stream_handle()
        buckets = []
        for lo, hi, early in sync.wait_each():
            if early is not None:            # (the reduction was waited for on the collectives' launch stream)
                ops.stream_wait(cur, C.c_void_p(early.cuda_stream))
            buckets.append((lo, hi))
        assert sum(hi - lo for lo, hi in buckets) == flat.numel(), 'gradient buckets do not cover the parameter buffer'
        first = True
        for lo, hi in buckets:
            a, b = sync.my_slice(lo, hi)
            if b > a:
                rs = [(a, b, 0)] if self._all_live else self.trainable_ranges(a, b)
                first = self._clip_accumulate(sync.grad_slice(g, lo, hi), [(x - a, y - x) for x, y, *_ in rs], first)
        everywhere = not (sync.sharded and sync.real_world > 1 and dist.is_initialized())
        if first:
            if everywhere:                   # (nothing trainable at all)
                self._clip_nothing()
                for lo, hi in buckets:
                    self._lerp(flat, *sync.my_slice(lo, hi))
                return
            ops.zero_(self._clip_sq)         # (nothing trainable in this rank's slices)
        if not everywhere:
            dist.all_reduce(self._clip_sq, op=dist.ReduceOp.SUM, group=sync.group)
        # (the all-reduced double is the same on every rank: so are the coefficient, the flag and the count -- no further collective)
        if not everywhere or self._guard_now:
            self._finalize(None, 2, count=True)
        with self._scaled():
            for lo, hi in buckets:
                a, b = sync.my_slice(lo, hi)
                if b > a:
                    self._update(flat, sync.grad_slice(g, lo, hi), a, b, args, g_is_slice=True)
                sync.gather_params(lo, hi)
        sync.finish_gathers()

    def _sync_state_steps(self):
        """``state[p]['step']`` tensors are refreshed when somebody looks (state_dict), not 38 times a step."""
        S = self._read_skipped()          # (one read, behind the joined streams; every counter stays as it is)
        got = self.steps_at(self._step_cut(), S)
        count = {id(p): k for p, k in zip(self.model._plist, got)}
        for p, st in self.state.items():
            st['step'] = torch.tensor(float(count.get(id(p), self._step)))
        return got

    # -- the state at a cut: host integers now, the buffers' values from wherever they were copied to ---------------------------
    def packed_param_groups(self):
        """``param_groups`` as ``state_dict()`` carries them: every key but ``'params'`` as it is, the parameters by their number"""
        number, groups = {}, []
        for grp in self.param_groups:
            for p in grp['params']:
                number.setdefault(id(p), len(number))
            groups.append(dict({k: v for k, v in grp.items() if k != 'params'}, params=[number[id(p)] for p in grp['params']]))
        return groups

    def host_cut(self, groups=True):
        """every HOST integer that, beside the values of the flat buffers and the device count of skipped steps, defines
        ``state_dict()``, ``ema_updates()``, ``skipped_total()`` and ``window_state()`` at this moment -- no device call.  With
        ``groups``: the packed ``param_groups``, deep-copied (a scheduler moves the learning rates on)."""
        import copy
        cut = self._step_cut()
        cut['ema'] = {'decay': self._ema_decay, 'done': self._ema_done, 'calls': self._ema_calls, 'skip_base': self._ema_skip_base}
        cut['window'] = {'phase': int(self._accum_phase), 'k': int(self._accum_k)}
        if groups:
            cut['param_groups'] = copy.deepcopy(self.packed_param_groups())
        return cut

    def _step_cut(self):
        """the part of ``host_cut()`` the per-parameter steps and the skipped total are made of"""
        return {'step': int(self._step), 'lags': [self._lag.get(n, 0) for n in self._names], 'flags': self._flags(),
                'guard_flags': None if self._guard_flags is None or self._skipped_dev is None else tuple(self._guard_flags),
                'skipped_folded': int(self._skipped_folded)}

    @classmethod
    def steps_at(cls, cut, skipped):
        """the per-parameter ``step`` of ``state_dict()``, in ``model.named_parameters()`` order, from ``host_cut()`` and the
        device count of skipped steps (counted only while a guarded step has run since the last fold)"""
        S = skipped if cut['guard_flags'] is not None else 0
        return cls.updates_received(cut['step'], cut['lags'], cut['guard_flags'] if S else cut['flags'], S)

    @staticmethod
    def skipped_total_at(cut, skipped):
        return cut['skipped_folded'] + (skipped if cut['guard_flags'] is not None else 0)

    def state_layout(self):
        """what ``state_dict_from`` needs of the optimiser, taken once: [(parameter number, index in ``named_parameters()``
        order, offset, numel, shape)] in the order of ``state``'s entries"""
        number = {}
        for grp in self.param_groups:
            for p in grp['params']:
                number.setdefault(id(p), len(number))
        at = {id(p): (i,) + tuple(self.model._offsets[n]) for i, (n, p) in enumerate(zip(self._names, self.model._plist))}
        return [(number[id(p)],) + at[id(p)] + (tuple(p.shape),) for p in self.state]

    def state_dict_from(self, m, v, steps, param_groups, layout=None):
        """``state_dict()`` over the flat moments ``m`` / ``v`` (this optimiser's, or host copies laid out the same), the
        per-parameter ``steps`` (``steps_at``) and packed ``param_groups``: torch.optim.Optimizer's layout -- the state by
        parameter number, in this optimiser's own order of entries; every tensor a view of the buffer it was given.  With a
        ``layout`` taken earlier (``state_layout()``) the optimiser itself is not looked at."""
        state = {}
        for number, i, off, k, shape in (self.state_layout() if layout is None else layout):
            state[number] = {'step': torch.tensor(float(steps[i])), 'exp_avg': m[off:off + k].view(shape),
                             'exp_avg_sq': v[off:off + k].view(shape)}
        return {'state': state, 'param_groups': param_groups}

    def consolidate_state(self):
        """COLLECTIVE (every rank must call it, at the same point): under the sharded data-parallel update a rank's moments are
        current on its own slices only; this all-gathers the others, after which ``state_dict()`` is complete on every rank.
        ``lirec_amd.util.save_checkpoint`` and ``lirec_amd.train.training`` call it before they read the state; a rank-0-only
        ``state_dict()`` never communicates (it would deadlock) -- it warns when the moments are stale."""
        self._ensure_state()
        sync = getattr(self.model, 'grad_sync', None)
        if sync is not None and sync.sharded and sync.real_world > 1:
            for lo, hi in sync.ranges:
                sync.gather(self._m, lo, hi)
                sync.gather(self._v, lo, hi)
                if self._ema is not None:
                    sync.gather(self._ema, lo, hi)
            sync.finish_gathers()
        self._consolidated_at = self._step

    def state_dict(self):
        self._ensure_state()
        self._join_side()       # (a replayed step may have left the first bucket's update running on the side stream)
        steps = self._sync_state_steps()
        sync = getattr(self.model, 'grad_sync', None)
        if sync is not None and sync.sharded and sync.real_world > 1 and getattr(self, '_consolidated_at', None) != self._step:
            import warnings
            warnings.warn('FusedAdam.state_dict(): sharded data-parallel update -- the moments outside this rank\'s slices are stale; '
                          'call optimizer.consolidate_state() on EVERY rank first (a collective)', RuntimeWarning, stacklevel=2)
        return self.state_dict_from(self._m, self._v, steps, self.packed_param_groups())

    def load_state_dict(self, state_dict):
        if any(g.get('amsgrad') for g in state_dict.get('param_groups', ())):
            raise ValueError('FusedAdam: amsgrad checkpoints are not supported (the reference never sets it, mlp/model.py:599-601)')
        if any(g.get('decoupled_weight_decay') for g in state_dict.get('param_groups', ())) and not self.device_hyper \
                and self._device_hyper_arg is not None:
            raise ValueError('FusedAdam.load_state_dict: the state has groups with decoupled_weight_decay (AdamW), which need '
                             'device_hyper, and device_hyper=False was asked for')
        self._ema_done, self._ema_calls = self.ema_updates(), 0      # (the device count of skipped steps is about to be zeroed)
        super().load_state_dict(state_dict)
        for grp in self.param_groups:        # (a state written before the key existed: coupled)
            grp.setdefault('decoupled_weight_decay', False)
        self.resolve_device_hyper()          # (decoupled groups switch the table route on)
        steps = [float(st['step']) for st in self.state.values() if 'step' in st]
        self._step = int(max(steps)) if steps else 0
        # (one step per parameter, as torch.optim.Adam keeps it: the ones behind the furthest carry the difference as their lag;
        #  a parameter without state has received no update)
        self._lag = {}
        self._guard_flags = None            # (the loaded steps are whole: nothing skipped on top of them)
        if self._skipped_dev is not None:
            self._skipped_dev.zero_()
        for n, p in zip(self._names, self.model._plist):
            st = self.state.get(p)
            lag = self._step - (int(float(st['step'])) if st and 'step' in st else 0)
            if lag:
                self._lag[n] = lag
        self._ranges_key = None
        self._m = None                      # re-flatten the loaded per-parameter moments
        self._ensure_state()
        self._ema_skip_base = self.skipped_total()
