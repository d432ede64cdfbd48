"""Training loop -- the ``mlp/train.py`` entry point on the HIP path.

``training(train_dataset, model=, loss=, optimizer=, val_dataset=|test_dataset=, ...)`` keeps the
reference's keyword protocol (mlp/train.py:21-27; both spellings of the validation kwarg are
accepted because the reference's recipes pass ``test_dataset=`` while the loop reads
``val_dataset``), its epoch structure (periodic eval every ``opt.test_fr`` epochs,
best-k checkpoint keeper, final ``%d.pth.tar``) and its per-10-iteration log line, plus clips/s.
Under ``torch.distributed`` (one process per GPU; wrap model / optimizer with ``lirec_amd.parallel.DataParallel`` first) the loop
is rank-aware: each rank draws its piece of every global batch (``parallel.ShardSampler`` unless a ``sampler=`` is given),
evaluation is sharded and reduced (``lirec_amd.test.testing``), every rank takes the same keep-this-checkpoint decision
(rank 0's, broadcast), the optimiser state is consolidated by all ranks and the files are written by rank 0 alone.
"""
from __future__ import annotations

import contextlib
import copy
import os
import math
import random
import time
from datetime import datetime

import torch

from . import parallel
from .config import opt
from .features import CLIP_WEIGHT, PinnedPool
from .loader import BlockLoader, ResidentLoader, make_loader
from .test import testing
from .util import AsyncCheckpointer, Averaging, ModelSaver, ema_entry, load_train_state, save_checkpoint


_COPY_STREAMS = {}
_print = print
_DP_RECORD_TRIES = 6          # data parallel: iterations 3 .. 8 of an epoch are where the ranks may agree to record the step


def _flush_losses(pending, losses, wait=True, finite_only=False):
    """Read queued per-iteration losses back in one transfer and feed the running average in order.  ``wait=False`` (the
    per-10-iteration log line): only the losses of steps the GPU has FINISHED are read, on a stream of their own -- a copy on
    the step's stream would wait for every step enqueued so far, i.e. drain the pipeline every ten iterations (measured: ~10 %
    of the loop); the printed value then lags the loop by the steps still in flight.  ``wait=True`` (epoch end): everything.
    ``finite_only`` (FusedAdam.skip_nonfinite): a NaN / Inf loss value -- a step the optimiser skipped -- stays out of the average."""
    if not pending:
        return
    k = len(pending)
    if not wait:
        k = 0
        while k < len(pending) and (pending[k][2] is None or pending[k][2].query()):
            k += 1
        if k == 0:
            return
    take = pending[:k]
    dev = take[0][0].device
    on_side = dev.type == 'cuda' and not wait
    with torch.cuda.stream(_COPY_STREAMS.setdefault(dev, torch.cuda.Stream(device=dev))) if on_side else contextlib.nullcontext():
        vals = torch.cat([v for v, _, _ in take]).cpu().tolist()
    for v, (_, n, _) in zip(vals, take):
        if finite_only and not math.isfinite(v):
            continue
        losses.update(v, n)
    del pending[:k]


def _flag_key(optimizer=None):
    """what a recorded step has baked in: the recipe flags and the optimiser's hyper-parameters (an LR schedule that changes
    `param_groups[0]['lr']` between epochs makes the loop record the step again)"""
    hyper = ()
    if optimizer is not None and getattr(optimizer, 'param_groups', None):
        from .graph import RecordedTrainStep
        hyper = RecordedTrainStep.hyper_key(optimizer)
    return repr((sorted((k, v) for k, v in opt.__dict__.items() if isinstance(v, (bool, int, float, str))), hyper))


def _recordable(model, batch) -> bool:
    """May this loader batch be stepped on by a recorded train step?  (opt.recorded_training; a CUDA model of the hot path; the
    batch's tensors in one device buffer -- features.batch_to_device -- with its pieces in the resident store.)  Under data
    parallelism this is one rank's view: the loop takes the decision for all ranks (`_all_ranks`).
    Second form -- a batch of a resident BLOCK store (lirec_amd.loader.BlockLoader), when ``opt.record_block_store`` asks for it:
    one process, the batch's tensors in one device buffer of a static layout, its features a two-plane ``Q32Block`` that names
    its samples, the gathered q32b layer-1 kernels in force (``opt.layer1_planes``, GEMM mode 2).  Anything else steps eagerly."""
    if not (bool(getattr(opt, 'recorded_training', True)) and '_dev_blob' in batch and hasattr(model, '_run_forward')
            and model.flat_params().is_cuda and getattr(opt, 'layer1_planes', False)):
        return False
    if 'piece_store' in batch:
        return bool(getattr(opt, 'pieces_gather', True) and getattr(opt, 'pieces_q32b', False))
    from . import ops
    f = batch.get('features')
    return bool(_block_store_mode()) and parallel.world_info()[1] == 1 and '_layout' in batch and \
        isinstance(f, ops.Q32Block) and f.clip_ids is not None and f.planes == 2 and ops.get_gemm_mode() == 2


def _block_store_mode() -> str:
    """``opt.record_block_store``, checked: '' (eager steps over a block store), 'bind' or 'list'"""
    mode = getattr(opt, 'record_block_store', '')
    if mode not in ('', 'bind', 'list'):
        raise ValueError('opt.record_block_store must be \'\', \'bind\' or \'list\', not %r' % (mode,))
    return mode


def _all_ranks(flag: bool, world: int) -> bool:
    """``flag`` on EVERY rank (one all-reduce(MIN) of a byte; every rank calls it at the same point of the loop).  The record /
    fall-back decisions of the data-parallel loop go through here: a rank that recorded, or fell back, alone would meet the
    others in different collectives (an advisor finding of round 4)."""
    if world <= 1:
        return bool(flag)
    import torch.distributed as dist
    from .parallel import _coll_device
    t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=_coll_device())
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(int(t.item()))


class _Stepper:
    """The optimiser step on every batch of one ``training()`` call, and what decides how it is taken.  A loader batch whose small
    tensors all live in ONE buffer of a layout that repeats from batch to batch (a resident piece store: lirec_amd.features.collate,
    static_layout) is stepped on by a RECORDED train step (lirec_amd.graph): the step's launches re-issued from C for ~0.1 ms of
    host time instead of ~0.6 ms of Python -- the loop is host-bound otherwise.  Recorded once, on the fourth such batch in a row
    (that batch's own, single step); a batch of another layout (the last, short one of an epoch) takes the eager step.
    A device-collating loader (``binds``) writes a batch of the recorded layout straight into the step's inputs; over a block store
    under ``opt.record_block_store = 'list'`` the recorded list draws its batch itself (``in_list``; BlockLoader.collate_at).
    State: ``recorded`` (None: no step is) with its ``layout``, ``blob`` (input buffer), ``flags`` (the ``_flag_key`` it has baked
    in) and ``released``; ``run`` batches in a row had ``last_layout``; ``run_barred``: a recording failed in this run, none is tried
    before the layout changes; ``overwrite_ok``: the coverage check's verdicts by (layout, flag key) -- a flag flip (:49-51) may
    route a parameter's gradient differently; ``dp_gave_up``: the ranks did not all record, and do not ask again."""

    def __init__(self, model, loss, optimizer, world, loader, stats, to_device=None, say=_print):
        self.model, self.loss, self.optimizer, self.world, self.loader, self.stats = model, loss, optimizer, world, loader, stats
        self.to_device, self.say, self.binds = to_device, say, isinstance(loader, (ResidentLoader, BlockLoader))
        self.in_list = False              # (the recorded step draws its batch itself: opt.record_block_store = 'list')
        self.recorded = self.layout = self.blob = self.flags = self.last_layout = None
        self.released = self.run_barred = self.dp_gave_up = False
        self.run, self.overwrite_ok = 0, {}

    def _forget(self):                    # (a recipe flag or a hyper-parameter the step has baked in changed: eager until recorded again)
        self.recorded.release()
        self.recorded, self.run, self.run_barred = None, 0, False

    def begin_epoch(self):
        if isinstance(self.loader, BlockLoader):
            # (a list that draws its own batches reads the epoch's ids at ONE address: asked for before the epoch is drawn)
            self.loader.stable_ids = _block_store_mode() == 'list' and self.world == 1
        if self.recorded is not None and self.flags != _flag_key(self.optimizer):      # (a recipe flag changed, :49-51)
            self._forget()

    def before_draw(self):
        """a device-collating loader is told before every draw where the recorded step's inputs are, so that a batch of that
        layout is written there -- behind the previous replay on this stream -- and nowhere else"""
        if self.binds and self.recorded is not None and self.in_list:
            self.loader.bind(self.layout, self.blob, in_list=True)
        elif self.binds and self.recorded is not None:
            self.loader.bind(self.layout, self.blob)
        elif self.binds:
            self.loader.unbind()

    def close(self):
        if self.recorded is not None:
            self.recorded.release()       # (back to the eager loop's way of passing the dropout key and Adam's step)
        if getattr(self.optimizer, 'accum_phase', 0):
            self.optimizer.drop_window()  # (a partial window at the end of training() is dropped: its micro-batches update nothing)

    def step(self, i, batch):
        """this batch's step: (loss value -- one element, on the device, not read --, labels); None: a one-label batch, skipped (:55-56)"""
        lay = tuple(batch.get('_layout', ())) if isinstance(batch, dict) else ()
        if self.recorded is not None and self.recorded.hyper_key(self.optimizer) != self.recorded._hyper:
            self._forget()                # (the learning rate changed inside the epoch)
        if self.recorded is not None and lay == self.layout:
            return self._replay(batch), len(batch['labels'])
        if isinstance(self.loader, BlockLoader) and self.loader.last_in_list:
            batch = self.loader.materialise(batch)      # (handed out for a list that will not run -- the step was forgotten: collated now)
        if self.to_device is not None:
            batch = self.to_device(batch)     # (every small tensor of the batch in ONE host-to-device copy: features.collate)
        n = len(batch['labels'])
        if n == 1:
            return None
        if self.recorded is not None and not self.released:
            self.recorded.release()       # an eager step in between: dropout key and Adam's step by value again
            self.released = True
        lval = self._record(batch, lay) if self.recorded is None and self._record_now(i, batch, lay) else None
        if lval is None:
            if lay and lay == self.last_layout:
                self.run += 1
            else:
                self.run, self.run_barred = (1 if lay else 0), False
            self.last_layout = lay
            # (a route that never overwrites -- FusedAdam.route, gradient accumulation: no coverage check -- it fills the gradient
            #  buffer, which holds the open window; an optimiser without a route: the check as ever)
            if self.recorded is None and lay and self.run == 3 and not self.run_barred and \
                    (not hasattr(self.optimizer, 'route') or self.optimizer.route().may_overwrite) and \
                    (lay, _flag_key(self.optimizer)) not in self.overwrite_ok and _recordable(self.model, batch):
                lval = self._checked(batch, lay)
            else:
                lval = self._eager(batch)
        return lval, n

    def _record_now(self, i, batch, lay) -> bool:
        """the fourth batch in a row of its layout?  Data parallel: the ranks step in lock-step (ShardSampler: the same number of
        batches of the same sizes), so iteration i is the same point of the program everywhere -- the decision is taken there, by all
        ranks together, a few iterations per epoch at most (one tiny all-reduce each) until the step is recorded or given up"""
        want = bool(lay and _recordable(self.model, batch) and self.run >= 3 and not self.run_barred and lay == self.last_layout)
        if self.world > 1:
            if self.dp_gave_up or not 3 <= i < 3 + _DP_RECORD_TRIES:
                return False
            want = _all_ranks(want, self.world)
            if not want and i == 3 + _DP_RECORD_TRIES - 1:
                self.dp_gave_up = True
        return want

    def _record(self, batch, lay):
        """this batch's step, recorded: its loss value -- None when it could not be (RecordedTrainStep undoes its own state: device
        counters detached, side stream joined; the eager step gives the same numbers).  Data parallel: a rank that recorded while another
        could not releases its step -- replaying alone, its collectives would come from other positions -- the step taken all the same."""
        from .graph import RecordedTrainStep
        lval = None
        # (a block store under opt.record_block_store = 'list': the list begins with the launches that draw its batch at the loader's
        #  device cursor -- set here to this batch, which the recording step then writes once more, the same bytes)
        # (a loss that converts the batch's labels on the host's side in front of every replay -- the cross-entropy loss's int32
        #  copies, loss.before_replay -- would read the buffer BEFORE the list has drawn the batch: such a step is recorded as
        #  under 'bind', the batch written by the loader's call)
        host_reads = getattr(self.loss, 'needs_before_replay', None)
        in_list = isinstance(self.loader, BlockLoader) and _block_store_mode() == 'list' and self.loader.can_draw_last_in_list() and \
            not (host_reads is not None and host_reads())
        draw = None
        if in_list:
            self.loader.cursor_to_last()
            loader, blob = self.loader, batch['_dev_blob']
            draw = lambda: loader.collate_at(lay, blob)
        extra = {'draw': draw} if draw is not None else {}      # (only when asked for: the call every other path makes is what it was)
        try:
            g = RecordedTrainStep(self.model, self.loss, self.optimizer, batch, warmup=0,
                                  overwrite=self.overwrite_ok.get((lay, _flag_key(self.optimizer))), **extra)
            self.recorded, self.layout, self.blob, self.flags, self.released = g, lay, batch['_dev_blob'], _flag_key(self.optimizer), False
            self.in_list = in_list
            lval = g.loss_out.clone()
        except Exception as e:
            self.say('recorded train step not used: %s' % str(e)[:160])
            self.recorded, self.run_barred = None, True
        if self.world > 1 and not _all_ranks(self.recorded is not None, self.world):
            if self.recorded is not None:
                self.recorded.release()
            self.recorded, self.run_barred, self.dp_gave_up = None, True, True
        return lval

    def _replay(self, batch):
        if self.released:
            self.recorded.resume()
            self.released = False
        assert not self.in_list or batch.get('_dev_blob') is self.blob, 'a list that draws its own batch runs on its bound buffer only'
        if batch.get('_dev_blob') is not self.blob:       # (else the loader wrote the batch into the step's inputs: nothing to copy)
            # (a host buffer -- or, a device-collated batch that was not written in place, its device buffer: one copy on this stream)
            self.blob.copy_(batch['_blob'] if '_blob' in batch else batch['_dev_blob'], non_blocking=True)
            PinnedPool.copied(batch.get('_slots'))
            self.stats['input_copies'] += 1
        self.stats['replays'] += 1
        return self.recorded.step().clone()

    def _checked(self, batch, lay):
        """the step before the recorded one: this batch's own, with the gradient-overwrite coverage check on it -- the recorded step
        may then skip the 76 MB zeroing pass and leave the side stream un-joined, like the benchmark's; same bits as the plain step"""
        from .graph import checked_overwrite_step
        ok, lv = checked_overwrite_step(self.model, self.loss, self.optimizer, batch)
        self.overwrite_ok[(lay, _flag_key(self.optimizer))] = ok
        return lv.detach().reshape(-1)[:1]

    def _eager(self, batch):
        out = self.model(batch)
        if self.to_device is None and isinstance(batch, dict) and batch.get('_slots'):
            PinnedPool.copied(batch['_slots'])       # (the model moved the pooled tables itself: hand the buffers back)
        lv = self.loss(out, batch)
        # the reference reads the loss back every iteration (``.item()``, :59): one host sync per step.  Here
        # the values are kept on the device and read back where they are printed (every 10th iteration, epoch end).
        lval = lv.detach().reshape(-1)[:1]
        self.optimizer.zero_grad()
        lv.backward()                     # a 0-d or one-element tensor, as mlp/train.py:62
        self.optimizer.step()
        return lval


def _check_distributed(train_dataset, model, loss, sampler, world):
    """(train_dataset, sampler) as the loop draws them -- this rank's shard sampler, class-balance weights --, or why the ranks do not add up"""
    if world > 1 and sampler is None:
        if getattr(model, 'grad_sync', None) is None:
            raise RuntimeError('training() under torch.distributed: wrap model / optimizer with lirec_amd.parallel.DataParallel first')
        sampler = parallel.ShardSampler(len(train_dataset), opt.batch_size, shuffle=True, seed=int(getattr(opt, 'seed', 0)), pad=True)
    if world > 1 and getattr(loss, 'dp_valid_mean', False) and getattr(loss, '_dp', None) is None:
        # (MultiTaskMaxMargin / MultiTaskCrossEntropyLoss: a mean over the clips that carry a relationship label, mlp/model.py:404-418 --
        #  a mean of per-rank means is not the global mean; attached, the loss divides by the all-reduced count)
        raise RuntimeError('training() under torch.distributed with %s: attach the loss -- DataParallel(model, optimizer, loss=loss) -- '
                           'so that its valid-row mean is the global batch\'s' % type(loss).__name__)
    if getattr(opt, 'class_balance', ''):
        # class-balanced training: every clip weighted by the frequency of its interaction class in the train set; the weights ride in
        # the batch (batch['clip_weight']) and are applied inside the loss kernel
        from .data import class_balanced_weights, interaction_labels, with_clip_weights
        train_dataset = with_clip_weights(train_dataset, class_balanced_weights(interaction_labels(train_dataset), train_dataset.n_classes,
                                                                                how=opt.class_balance))
    weighted = CLIP_WEIGHT in (getattr(train_dataset, '_stacked', None) or ()) or getattr(train_dataset, 'carries_clip_weights', False)
    if world > 1 and weighted and getattr(opt, 'clip_weight_norm', 'sum') == 'sum' and getattr(loss, '_dp', None) is None:
        # (a weighted mean divides by the GLOBAL batch's weight sums: the ranks' own sums differ even with even batches)
        raise RuntimeError('training() under torch.distributed with clip weights and clip_weight_norm=\'sum\': attach the loss -- '
                           'DataParallel(model, optimizer, loss=loss) -- so that its weighted mean is the global batch\'s')
    return train_dataset, sampler


# ---------------------------------------------------------------------------
# continuing a run (DESIGN "Continuing a run")
# ---------------------------------------------------------------------------

# opt fields that steer the loop, its logs, its files and the launch form -- every launch form gives the eager loop's bits -- but no
# step's numbers: the two halves of a continued run may differ in them.  Every other plain field of opt is in the fingerprint.
_LOOP_FIELDS = frozenset((
    'epochs', 'store_root', 'resume', 'resume_train', 'resume_str', 'model_name', 'log_prefix', 'save_model', 'save_model_often',
    'save_train_state', 'checkpoint_every', 'checkpoint_async', 'test', 'test_fr', 'num_workers', 'device', 'sanity_check', 'param_stats_every',
    'tr_sum_max_flag', 'recorded_training', 'record_block_store', 'record_eval', 'device_collate', 'device_metrics', 'dp_shard_eval',
    'strict'))


def _hyper_fingerprint(optimizer):
    """what of the optimiser must not differ between the halves of a continued run: ``RecordedTrainStep.hyper_key`` without the
    learning rates (the scheduler moves them; the checkpoint's are loaded) and without the lags (state, which is loaded too) --
    betas, eps, weight decay, the groups' membership, the frozen set, clip, guard, average and accumulation.  An optimiser that is
    not a FusedAdam: its groups' settings but ``lr``."""
    if not hasattr(optimizer, 'frozen_key'):
        return repr([sorted((k, repr(v)) for k, v in g.items() if k not in ('params', 'lr', 'initial_lr'))
                     for g in optimizer.param_groups])
    from .graph import RecordedTrainStep
    key, frozen = RecordedTrainStep.hyper_key(optimizer), optimizer.frozen_key()
    if not getattr(optimizer, 'device_hyper', False):
        key = key[1:]                     # (by value the key begins with the first group's lr)
    else:
        rows = [(tuple(float(b) for b in g['betas']), float(g['eps']), float(g['weight_decay']), bool(g.get('decoupled_weight_decay')))
                for g in optimizer.param_groups]
        key = key + (('groups', tuple(rows)),)      # (in device tables, not in the key: compared here)
    key = tuple(k for k in key if not (frozen and k == frozen))
    return repr(key + (('requires_grad', tuple(bool(p.requires_grad) for p in optimizer.model._plist)),))


def fingerprint(train_dataset, model, optimizer) -> dict:
    """{field: value} of everything that must be the same in both halves of a continued run"""
    fp = {'batch_size': int(opt.batch_size), 'dropout': float(opt.dropout), 'dropout_seed': int(opt.dropout_seed),
          'accumulate_steps': int(getattr(optimizer, 'accumulate_steps', 1))}
    for k, v in sorted(opt.__dict__.items()):
        if isinstance(v, (bool, int, float, str)) and k not in _LOOP_FIELDS and k not in fp:
            fp['opt.' + k] = v
    fp['optimizer'] = _hyper_fingerprint(optimizer)
    fp['len(train_dataset)'] = len(train_dataset)
    fp['parameter names'] = [n for n, _ in model.named_parameters()]
    return fp


class TrainState:
    """What defines the NEXT step of a ``training()`` call beside the model's and the optimiser's ``state_dict()`` -- the one place
    that knows: ``capture`` reads it, ``as_dict`` is ``ck['train_state']`` (plain Python, numpy and CPU tensors), ``from_dict``
    checks the version, ``check`` the fingerprint, ``restore`` puts it back.  A feature that adds state to a step adds a field here.

    Version 1: ``epoch`` (the epoch in progress), ``batches_done`` (loader batches of it already consumed; 0: the epoch starts),
    ``steps_taken``, ``seen`` and ``loss_sum`` / ``loss_count`` (the cut epoch's clip count and loss average), ``dropout_calls``,
    ``sample_calls`` (the host mirrors: current under a recorded step, no device read), ``skipped_total`` (the one device read),
    ``window`` (FusedAdam.window_state), ``scheduler``, ``rng`` ({'torch', 'numpy', 'python'} at capture) and ``epoch_rng`` (torch's
    just before the running epoch's ``iter(loader)``: its permutation is drawn from it), ``tr_sum_max_flag``, ``start``, ``saver``
    (ModelSaver.state_dict) and ``fingerprint``."""
    VERSION = 1

    def __init__(self, **fields):
        self.__dict__.update(fields)

    @classmethod
    def capture(cls, train_dataset, model, loss, optimizer, scheduler=None, saver=None, *, epoch, batches_done, steps_taken, seen,
                losses, epoch_rng, start, device_reads=True):
        """``device_reads=False`` (the asynchronous rolling checkpoint): the two fields that read the device -- ``skipped_total`` and
        ``window`` -- are left None for ``AsyncCheckpointer``, which fills them in from its snapshot; everything else is taken here"""
        import numpy as np
        return cls(version=cls.VERSION, epoch=int(epoch), batches_done=int(batches_done), steps_taken=int(steps_taken), seen=int(seen),
                   loss_sum=losses.sum, loss_count=losses.count,
                   dropout_calls=int(getattr(model, 'dropout_calls', 0)), sample_calls=int(getattr(loss, 'sample_calls', 0)),
                   skipped_total=(int(optimizer.skipped_total()) if hasattr(optimizer, 'skipped_total') else 0) if device_reads else None,
                   window=(optimizer.window_state() if hasattr(optimizer, 'window_state') else None) if device_reads else None,
                   scheduler=copy.deepcopy(scheduler.state_dict()) if scheduler is not None else None,
                   rng={'torch': torch.get_rng_state(), 'numpy': np.random.get_state(), 'python': random.getstate()},
                   epoch_rng=epoch_rng, tr_sum_max_flag=bool(opt.tr_sum_max_flag), start=start,
                   saver=saver.state_dict() if saver is not None else None,
                   fingerprint=fingerprint(train_dataset, model, optimizer))

    def as_dict(self) -> dict:
        return dict(self.__dict__)

    @classmethod
    def from_dict(cls, d):
        if not isinstance(d, dict) or d.get('version') != cls.VERSION:
            raise ValueError('train state of version %r: this build reads version %d only' % (d.get('version') if isinstance(d, dict) else d, cls.VERSION))
        return cls(**d)

    def check(self, train_dataset, model, optimizer):
        """ValueError naming the first field in which this run is not the checkpoint's"""
        now = fingerprint(train_dataset, model, optimizer)
        for k in list(self.fingerprint) + [k for k in now if k not in self.fingerprint]:
            if k not in now or k not in self.fingerprint or now[k] != self.fingerprint[k]:
                raise ValueError('training(resume=): %s differs -- the checkpoint was written with %r, this run has %r'
                                 % (k, self.fingerprint.get(k, '<absent>'), now.get(k, '<absent>')))

    def restore_rng(self):
        import numpy as np
        torch.set_rng_state(self.rng['torch'])
        np.random.set_state(self.rng['numpy'])
        random.setstate(self.rng['python'])

    def restore(self, ck, model, loss, optimizer, scheduler=None, saver=None, losses=None, world=1):
        """the checkpoint ``ck`` and this state into freshly built objects: model, optimiser (state_dict, then what is outside it:
        the skipped count, the average, the open window), scheduler, the call counters, ``opt.tr_sum_max_flag``, the kept-metric
        history, the cut epoch's loss average, the RNGs as they were at capture"""
        model.load_state_dict(ck['state_dict'])
        optimizer.load_state_dict(ck['optimizer'])
        if hasattr(optimizer, 'continue_skipped_from'):
            optimizer.continue_skipped_from(self.skipped_total)
        if 'ema' in ck and hasattr(optimizer, 'load_ema_state_dict'):
            optimizer.load_ema_state_dict(ck['ema']['state_dict'], updates=ck['ema'].get('updates'))
        if self.window is not None and self.window['phase'] != 0:
            if world > 1:
                raise ValueError('training(resume=): the checkpoint was taken inside an accumulation window; under torch.distributed '
                                 'the window\'s gradients are each rank\'s own and the file holds rank 0\'s only')
            optimizer.load_window_state(self.window)
        if (scheduler is None) != (self.scheduler is None):
            raise ValueError('training(resume=): scheduler differs -- the checkpoint was written %s one, this run has %s'
                             % (('without', 'one') if self.scheduler is None else ('with', 'none')))
        if scheduler is not None:
            scheduler.load_state_dict(copy.deepcopy(self.scheduler))
        if hasattr(model, 'dropout_calls'):
            model.dropout_calls = self.dropout_calls
        if hasattr(loss, 'sample_calls'):
            loss.sample_calls = self.sample_calls
        opt.tr_sum_max_flag = self.tr_sum_max_flag
        if saver is not None and self.saver is not None:
            saver.load_state_dict(self.saver)
        if losses is not None:
            losses.sum, losses.count = self.loss_sum, self.loss_count
            losses.avg = losses.sum / losses.count if losses.count else 0.0
        self.restore_rng()


def _iter_from(loader, start):
    """the epoch's batches from the ``start``-th on, the batch sampler drawn from the torch RNG as it is NOW and no sample of a batch
    passed over touched: the project's loaders have ``iter_from``; a stock ``DataLoader`` is drawn once over the bare indices --
    which consumes the RNG exactly as its own ``iter()`` does -- and built anew over the explicit remaining batch list."""
    if hasattr(loader, 'iter_from'):
        return loader.iter_from(start)
    DL = torch.utils.data.DataLoader
    drawn = list(DL(range(len(loader.dataset)), batch_sampler=loader.batch_sampler, num_workers=0, collate_fn=list))
    return iter(DL(loader.dataset, batch_sampler=drawn[start:], num_workers=loader.num_workers, collate_fn=loader.collate_fn,
                   pin_memory=loader.pin_memory))


def _evaluate_and_keep(epoch, start, train_dataset, val_dataset, test_dataset, model, loss, optimizer, saver, rank, world):
    """the periodic evaluation: the train set, then -- opt.test -- the validation set, whose metrics decide whether this epoch's
    checkpoint is kept (and the test set evaluated); returns whether it was.  COLLECTIVE under torch.distributed: every rank takes
    the same path."""
    testing(train_dataset, model, loss, total_iter=epoch, mode='train', train_start_time=start)
    if not (opt.test and val_dataset is not None):
        return False
    # (opt.eval_ema: val / test see the averaged weights -- FusedAdam.ema_weights: swapped in by value, the live ones restored bit for bit)
    averaged = getattr(opt, 'eval_ema', False) and getattr(optimizer, 'ema_decay', None) is not None
    eval_weights = optimizer.ema_weights if averaged else contextlib.nullcontext
    # (sharded + reduced under data parallelism: the same dict on every rank)
    if getattr(opt, 'eval_ema', False) and hasattr(optimizer, 'consolidate_state') and world > 1:
        optimizer.consolidate_state()         # (a collective: the shadow outside a rank's slices is stale otherwise)
    with eval_weights():
        check_val = testing(val_dataset, model, loss, total_iter=epoch, train_start_time=start, mode='val')
    keep = saver.check(check_val) if rank == 0 else False
    if world > 1:                             # rank 0 keeps the history the decision is taken against: its verdict, everywhere
        keep = bool(parallel.all_reduce_counters({'keep': int(keep)})['keep'])
    if not keep:
        return False
    if hasattr(optimizer, 'consolidate_state'):
        optimizer.consolidate_state()         # (a collective: every rank is here)
    if rank == 0:
        kept = {'epoch': epoch, 'state_dict': copy.deepcopy(model.state_dict()), 'optimizer': copy.deepcopy(optimizer.state_dict())}
        ema = ema_entry(optimizer)
        if ema is not None:
            kept['ema'] = copy.deepcopy(ema)
        saver.update(check_val, kept, epoch)
    if test_dataset is not None:
        with eval_weights():
            testing(test_dataset, model, loss, total_iter=epoch, train_start_time=start, mode='test')
    return True


def _print_param_stats(optimizer, say):
    """one line per parameter from ONE ``param_stats().host()`` read: the norms as the update sees them, the size of the last Adam
    step against the weight, and the non-finite counts where there are any (a frozen parameter has no gradient columns, a
    parameter never updated no ratio: '-')"""
    fmt = lambda x: '-' if x is None else '%.4e' % x
    say('parameter statistics (grad_norm, grad_absmax, param_norm, update_ratio):')
    for name, s in optimizer.param_stats().host().items():
        bad = ['%s %d' % (k, c) for k, c in (('grad', s.grad_nonfinite), ('param', s.param_nonfinite), ('update', s.update_nonfinite)) if c]
        say('  %-40s %s  %s  %s  %s%s' % (name, fmt(s.grad_norm), fmt(s.grad_absmax), fmt(s.param_norm), fmt(s.update_ratio),
                                         '  non-finite: ' + ', '.join(bad) if bad else ''))


def training(train_dataset, **kwargs):
    """``resume=`` (a path, or a loaded checkpoint dict; ``opt.resume_train`` with ``opt.resume_str`` set is the same): continue the
    run that wrote that checkpoint -- with ``opt.save_train_state`` or as the rolling file of ``opt.checkpoint_every`` -- on the
    bits of the run that was never cut.  The caller builds model, loss, optimiser, datasets and scheduler exactly as for the first
    run; everything is loaded here (``TrainState``).  A ``sampler=`` of the caller's own is the caller's to make resumable: the
    loop restores the RNGs and calls ``set_epoch``, nothing else."""
    rank, world = parallel.world_info()
    print = _print if rank == 0 else (lambda *a, **k: None)        # (one log, rank 0's)
    start = datetime.now().strftime('%Y%m%d-%H%M%S')
    print('set parameters and model, train start time: %s' % start)
    model, loss, optimizer = kwargs['model'], kwargs['loss'], kwargs['optimizer']
    resume = kwargs.get('resume')
    if resume is None and getattr(opt, 'resume_train', False) and getattr(opt, 'resume_str', ''):
        resume = opt.resume_str
    val_dataset = kwargs.get('val_dataset', kwargs.get('test_dataset'))
    test_dataset = kwargs.get('test_dataset') if 'val_dataset' in kwargs else None
    # scheduler= any object with .step() (torch.optim.lr_scheduler.*), called after every optimiser step -- eager or replayed --
    # (scheduler_every='step') or after every epoch ('epoch').  With FusedAdam(device_hyper=True) the recorded step follows it
    # without being recorded again (FusedAdam.sync_hyper); by value every change of the learning rate records anew.
    scheduler, scheduler_every = kwargs.get('scheduler'), kwargs.get('scheduler_every', 'step')
    if scheduler_every not in ('step', 'epoch'):
        raise ValueError('training(): scheduler_every must be \'step\' or \'epoch\', not %r' % (scheduler_every,))
    sched_step = scheduler.step if (scheduler is not None and scheduler_every == 'step') else (lambda: None)
    train_dataset, sampler = _check_distributed(train_dataset, model, loss, kwargs.get('sampler'), world)
    batch_time, data_time, losses = Averaging(), Averaging(), Averaging()
    guarded = lambda: bool(getattr(optimizer, 'skip_nonfinite', False))
    # (a dataset may bring its own collate_fn -- lirec_amd.features.PiecesDataset does --; with opt.device_collate over a resident store
    #  the batch buffer is written on the device from the sample ids and, once a step is recorded, straight into that step's inputs)
    loader = make_loader(train_dataset, opt.batch_size, shuffle=sampler is None, sampler=sampler)
    print('epochs: %s' % opt.epochs)
    saver = ModelSaver(path=opt.store_root) if rank == 0 else None      # (the kept checkpoints live on rank 0)
    epoch = -1
    # (what the last call did with its recorded step: replays, host- or device-side copies into its input buffer, and the loader)
    stats = training.last = {'replays': 0, 'input_copies': 0, 'loader': loader}
    to_dev = getattr(train_dataset, 'to_device', None) if str(opt.device).startswith('cuda') else None
    stepper = _Stepper(model, loss, optimizer, world, loader, stats, to_device=to_dev, say=print)
    # opt.param_stats_every = N: at the end of every N-th epoch one line per parameter (FusedAdam.param_stats: two launches and ONE
    # read); single process only -- under data parallelism one notice, and nothing else.  0 issues nothing.
    stats_every = int(getattr(opt, 'param_stats_every', 0) or 0) if hasattr(optimizer, 'param_stats') else 0
    if stats_every and max(world, getattr(getattr(model, 'grad_sync', None), 'world', 1)) > 1:
        print('param_stats_every: per-parameter statistics are single-process only (under data parallelism they would need '
              'collectives); ignored')
        stats_every = 0

    keep_state = bool(getattr(opt, 'save_train_state', False))
    every = int(getattr(opt, 'checkpoint_every', 0) or 0)
    if every and world > 1:
        print('checkpoint_every: the rolling checkpoint is single-process only (under data parallelism a cut inside an epoch is not '
              'continued); ignored')
        every = 0
    rolling = os.path.join(opt.store_root, 'last.pth.tar')
    first_epoch, resumed, steps_taken = 0, None, 0
    if resume is not None:
        ck, ts = load_train_state(resume)
        resumed = TrainState.from_dict(ts)
        resumed.check(train_dataset, model, optimizer)
        resumed.restore(ck, model, loss, optimizer, scheduler, saver, losses, world=world)
        first_epoch, steps_taken, start = resumed.epoch, resumed.steps_taken, resumed.start
        print('resumed at epoch %d, batch %d (%d steps taken; train start time: %s)' % (resumed.epoch, resumed.batches_done, steps_taken, start))
        if first_epoch >= opt.epochs:
            print('nothing to do: the checkpoint\'s run had finished its %d epochs' % opt.epochs)
            return model
        if opt.tr_sum_max and first_epoch > 20:           # (the flip at epoch 20 has happened, mlp/train.py:49-51)
            opt.tr_sum_max_flag = True

    def capture(epoch, batches_done, seen, epoch_rng, device_reads=True):
        return TrainState.capture(train_dataset, model, loss, optimizer, scheduler, saver, epoch=epoch, batches_done=batches_done,
                                  steps_taken=steps_taken, seen=seen, losses=losses, epoch_rng=epoch_rng, start=start,
                                  device_reads=device_reads).as_dict()

    # opt.checkpoint_async: the rolling file is cut by one launch and written behind the steps (lirec_amd.util.AsyncCheckpointer;
    # DESIGN 4.j2).  Off -- or with no rolling file to write -- nothing is made: no thread, no arena, no launch.
    writer = AsyncCheckpointer(model, optimizer) if (every and bool(getattr(opt, 'checkpoint_async', False))) else None

    def write_rolling(epoch, batches_done, seen, epoch_rng):
        if writer is not None:
            writer.save(rolling, epoch, capture(epoch, batches_done, seen, epoch_rng, device_reads=False))
        else:
            save_checkpoint(rolling, epoch, model, optimizer, train_state=capture(epoch, batches_done, seen, epoch_rng), atomic=True)

    def drained():
        if writer is not None:
            try:
                writer.close()
            finally:
                stats.update(checkpoint_writes=writer.stats['writes'], checkpoint_waits=writer.stats['waits'],
                             checkpoint_save_s=writer.stats['save_s'])

    def batches(it):
        while True:
            stepper.before_draw()
            try:
                yield next(it)
            except StopIteration:
                return
    epoch_rng = torch.get_rng_state()
    try:
        for epoch in range(first_epoch, opt.epochs):
            model.train()
            train_dataset.epoch = epoch
            if hasattr(sampler, 'set_epoch'):
                sampler.set_epoch(epoch)
            print('Epoch # %d' % epoch)
            if opt.tr_sum_max and epoch == 20:            # mlp/train.py:49-51
                opt.tr_sum_max_flag = True
            seen, end, t_epoch = 0, time.time(), time.time()
            pending = []
            stepper.begin_epoch()
            # (a run cut inside this epoch: the epoch's permutation drawn again from the RNG state it was drawn from, the batches already
            #  stepped on passed over untouched, then the RNG as it was at the cut)
            skip = resumed.batches_done if (resumed is not None and epoch == first_epoch) else 0
            if skip:
                torch.set_rng_state(resumed.epoch_rng)
                seen = resumed.seen
            if keep_state or every:
                epoch_rng = torch.get_rng_state()
            it = _iter_from(loader, skip) if skip else iter(loader)
            if skip:
                torch.set_rng_state(resumed.rng['torch'])
            since_write = 0
            for i, batch in enumerate(batches(it), skip):
                data_time.update(time.time() - end)
                took = stepper.step(i, batch)
                if took is None:
                    continue
                lval, n = took
                # (gradient accumulation: a scheduler counts UPDATES -- after a step() the phase is 0 exactly when that call applied)
                if getattr(optimizer, 'accum_phase', 0) == 0:
                    sched_step()
                ev = None
                if lval.is_cuda:
                    ev = torch.cuda.Event()
                    ev.record()
                pending.append((lval, n, ev))
                batch_time.update(time.time() - end)
                end = time.time()
                seen += n
                steps_taken += 1
                since_write += 1
                if every and since_write >= every:
                    _flush_losses(pending, losses, finite_only=guarded())
                    write_rolling(epoch, i + 1, seen, epoch_rng)
                    since_write = 0
                if i % 10 == 0 and i:
                    _flush_losses(pending, losses, wait=False, finite_only=guarded())
                    print('Epoch: [{0}][{1}/{2}]\tTime {bt.val:.3f} ({bt.avg:.3f})\tData {dt.val:.3f} ({dt.avg:.3f})\t'
                          'Loss {ls.val:.4f} ({ls.avg:.4f})\t'.format(epoch, i, len(loader), bt=batch_time, dt=data_time, ls=losses))
            _flush_losses(pending, losses, finite_only=guarded())
            if scheduler is not None and scheduler_every == 'epoch':
                scheduler.step()
            print(seen)
            print('loss: %f' % losses.avg)
            print('train clips/s: %.1f' % (seen / max(time.time() - t_epoch, 1e-9)))
            if guarded():
                print('skipped steps: %d' % optimizer.skipped_total())        # (one read per epoch)
            if stats_every and (epoch + 1) % stats_every == 0:
                _print_param_stats(optimizer, print)
            losses.reset()
            if epoch % opt.test_fr == 0:
                kept = _evaluate_and_keep(epoch, start, train_dataset, val_dataset, test_dataset, model, loss, optimizer, saver, rank, world)
                print(getattr(opt, 'log_prefix', ''))
                if kept and keep_state and rank == 0:
                    saver.save()              # (the kept checkpoints live in host memory until then: they survive an interruption)
            if opt.save_model and opt.save_model_often and epoch % 30 == 0 and rank == 0:
                saver.save()
            if every:                         # (the epoch is over: "epoch + 1, no batch done" -- the next epoch starts)
                write_rolling(epoch + 1, 0, 0, epoch_rng)
    finally:
        drained()            # (whatever ends the loop: no write in flight, no thread left; the writer's error is raised here)
    # (before close() drops a partial accumulation window: a run continued from the final checkpoint goes on inside it)
    final_state = capture(epoch + 1, 0, 0, epoch_rng) if (keep_state and opt.save_model) else None
    stepper.close()
    opt.resume_str = os.path.join(opt.store_root, '%d.pth.tar' % epoch)
    if opt.save_model:
        # (the flag off: the call is what it always was)
        save_checkpoint(opt.resume_str, epoch, model, optimizer, *(() if final_state is None else (final_state,)))
    return model


training.last = {}
