"""Small host helpers the loops use: running averages, best-k checkpoint keeper,
checkpoint load/save in the reference's dict layout.

Checkpoint format (mlp/train.py:84-87,102-106; utils/util_functions.py:274-291):
``{'epoch': int, 'state_dict': model.state_dict(), 'optimizer': optimizer.state_dict()}``
saved with ``torch.save``.  Keys and shapes of both state dicts are the reference's, so
its ``*.pth.tar`` files load here and ours load there.
"""
from __future__ import annotations

import os
import time
from collections import defaultdict

import torch

from .config import opt


class Averaging:
    """Last value + running weighted mean (utils/util_functions.py:23-38)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = 0.0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def timing(fn):
    """Print the wall time of a call (utils/util_functions.py:294-305)."""
    def wrapped(*a, **k):
        t0 = time.time()
        out = fn(*a, **k)
        dt = time.time() - t0
        print('%s took %0.3f ms ~ %0.3f min ~ %0.3f sec' % (fn, dt * 1e3, dt / 60.0, dt))
        return out
    return wrapped


def dir_check(path):
    if path and not os.path.exists(path):
        os.makedirs(path, exist_ok=True)


class ModelSaver:
    """Keeps the best ``n`` checkpoints per metric (utils/model_saver.py:17-64):
    ``check(values)`` says whether any metric beats its current worst kept value,
    ``update`` inserts and evicts, ``save`` writes ``<path>/<metric>/v%.4f_ep%d.pth.tar``."""

    def __init__(self, n=4, path=''):
        self.n, self.path = n, path
        self.eval = defaultdict(dict)        # metric -> {epoch: value}
        self.models = defaultdict(dict)      # metric -> {epoch: checkpoint dict}
        self.saved = defaultdict(dict)
        dir_check(path)

    def _worst(self, key):
        # ties resolve to the entry visited last, as the reference's <= scan does (:45-47)
        worst_ep, worst = None, None
        for ep, v in self.eval[key].items():
            if worst is None or v <= worst:
                worst_ep, worst = ep, v
        return worst_ep

    def check(self, val: dict) -> bool:
        for key, v in val.items():
            if len(self.eval[key]) < self.n:
                return True
            if v > self.eval[key][self._worst(key)]:
                return True
        return False

    def update(self, val, model, epoch):
        for key, v in val.items():
            if len(self.eval[key]) >= self.n:
                w = self._worst(key)
                self.eval[key].pop(w)
                self.models[key].pop(w, None)        # (an entry restored by load_state_dict lives in its file only)
                self.saved[key].pop(w, None)
            self.eval[key][epoch] = v
            self.models[key][epoch] = model
            assert len(self.eval[key]) <= self.n

    def save(self):
        for key in self.eval:
            d = os.path.join(self.path, key)
            dir_check(d)
            keep = set(self.saved[key].values())
            for fn in os.listdir(d):
                if os.path.join(d, fn) not in keep:
                    os.remove(os.path.join(d, fn))
            for epoch, v in self.eval[key].items():
                if epoch in self.saved[key] or epoch not in self.models[key]:
                    continue
                fn = os.path.join(d, 'v%.4f_ep%d.pth.tar' % (v, epoch))
                torch.save(self.models[key][epoch], fn)
                self.saved[key][epoch] = fn

    def state_dict(self):
        """what the keep-this-checkpoint decisions are taken against -- ``eval``, ``saved`` (the files written so far) and ``n`` -- as
        plain dicts whose order is the insertion order (``_worst`` resolves ties by it).  The kept checkpoint dicts themselves are
        not in it: they are on disk once ``save()`` has run."""
        return {'n': self.n, 'eval': {k: dict(v) for k, v in self.eval.items()}, 'saved': {k: dict(v) for k, v in self.saved.items()}}

    def load_state_dict(self, sd):
        """continue from ``state_dict()``: the same ``check()`` verdicts and evictions from here on.  A kept entry whose file was
        never written stays in the history but cannot be written later (its checkpoint dict is gone; ``save()`` passes it over) --
        ``training()`` with ``opt.save_train_state`` saves whenever the kept set changes, so that there is none."""
        self.n = int(sd['n'])
        self.eval, self.models, self.saved = defaultdict(dict), defaultdict(dict), defaultdict(dict)
        for k, v in sd['eval'].items():
            self.eval[k] = dict(v)
        for k, v in sd['saved'].items():
            self.saved[k] = dict(v)


def ema_entry(optimizer):
    """``ck['ema']`` of a checkpoint: {'decay', 'updates', 'state_dict'} of an optimiser whose weight average is on
    (FusedAdam.ema_decay), else None.  The state_dict has the model's keys and shapes: it loads into a model as it is."""
    if getattr(optimizer, 'ema_decay', None) is None or not hasattr(optimizer, 'ema_state_dict'):
        return None
    return ema_entry_from(optimizer.ema_decay, optimizer.ema_updates(), optimizer.ema_state_dict())


def ema_entry_from(decay, updates, state_dict):
    """``ema_entry`` from its three parts, wherever they were read"""
    return {'decay': float(decay), 'updates': int(updates), 'state_dict': state_dict}


def checkpoint_dict(epoch, state_dict, optimizer_state, group_names=None, ema=None, train_state=None):
    """the checkpoint's dict from its parts, in the order of keys ``save_checkpoint`` has always written"""
    ck = {'epoch': epoch, 'state_dict': state_dict, 'optimizer': optimizer_state}
    if group_names is not None:
        ck['param_group_names'] = group_names       # (who is in which group: checkpoint_to_flat needs it)
    if ema is not None:
        ck['ema'] = ema                 # (beside the optimizer state, which stays what a stock Adam loads)
    if train_state is not None:
        ck['train_state'] = train_state
    return ck


def _group_names(optimizer):
    if len(getattr(optimizer, 'param_groups', ())) > 1 and hasattr(optimizer, 'group_names'):
        return optimizer.group_names()
    return None


def write_atomic(ck, path):
    """``torch.save`` under a temporary name beside ``path``, moved into place by ``os.replace``: an interruption -- or an error --
    during the write leaves the previous file as it was"""
    tmp = '%s.tmp.%d' % (path, os.getpid())
    try:
        torch.save(ck, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def save_checkpoint(path, epoch, model, optimizer, train_state=None, atomic=False):
    """COLLECTIVE under torch.distributed (every rank calls it): the sharded update's moments are gathered by all ranks, the file
    is written by rank 0 alone, and nobody returns before it is on disk.  ``train_state`` (a dict: lirec_amd.train.TrainState):
    kept as ``ck['train_state']`` -- what ``training(resume=)`` continues from; None: the keys are what they always were.
    ``atomic``: written under a temporary name beside ``path`` and moved into place (``os.replace``): an interruption during the
    write leaves the previous file as it was."""
    import torch.distributed as dist
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    if hasattr(optimizer, 'consolidate_state'):
        optimizer.consolidate_state()
    if not multi or dist.get_rank() == 0:
        dir_check(os.path.dirname(path))
        ck = checkpoint_dict(epoch, model.state_dict(), optimizer.state_dict(), _group_names(optimizer), ema_entry(optimizer), train_state)
        if atomic:
            write_atomic(ck, path)
        else:
            torch.save(ck, path)
    if multi:
        dist.barrier()


class AsyncCheckpointer:
    """The rolling checkpoint written BEHIND the steps (``opt.checkpoint_async``).  ``save(path, epoch, train_state)``
    costs the loop one launch: it joins what ``state_dict()`` joins, copies the state's flat device buffers -- parameters, both
    moments, the average when on, the open accumulation window's gradients, the count of skipped steps -- into a device arena
    with ONE ``lirec_snapshot`` on the current stream, has a copy stream of its own bring the arena to pinned host memory behind
    an event, and returns.  A writer thread waits for that copy, checks every range against the digest the snapshot left on the
    device (a mismatch means arena or pinned memory was reused too early: RuntimeError), builds the dict ``save_checkpoint``
    builds -- through the same builders (``Model.state_dict_from``, ``FusedAdam.state_dict_from`` / ``steps_at`` /
    ``ema_updates_at`` / ``window_state_from``) over the host copies and the host integers taken at the cut -- and writes it
    under a temporary name moved into place.  The file loads (``map_location='cpu'``) to the tree of the synchronous file; its
    tensors were saved from host memory.  ``train_state``: the dict of ``TrainState.capture(..., device_reads=False)``; its two
    device-side fields (``skipped_total``, ``window``) are filled in from the snapshot.

    At most one write is in flight: a ``save()`` that finds the last one still running waits for it first (``stats['waits']``).
    An exception in the writer is raised from the next ``save()``, ``wait()`` or ``close()``; the previous file stays.
    ``close()`` drains, joins the thread and frees arena and pinned memory; idempotent.  The thread issues no launch and looks at
    neither model nor optimiser -- keys, shapes, offsets and host integers are taken in ``save()`` --, and none is alive between
    a ``wait()`` and the next ``save()``.  Single process only."""

    ALIGN = 256

    def __init__(self, model, optimizer):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError('AsyncCheckpointer: single process only (under torch.distributed the rolling checkpoint is not written)')
        if not (hasattr(model, 'state_dict_layout') and hasattr(optimizer, 'state_layout') and hasattr(optimizer, 'host_cut')):
            raise TypeError('AsyncCheckpointer needs a lirec_amd model over a flat parameter buffer and a FusedAdam, not %s / %s'
                            % (type(model).__name__, type(optimizer).__name__))
        self.model, self.optimizer = model, optimizer
        self.stats = {'writes': 0, 'waits': 0, 'save_s': 0.0, 'writer_s': 0.0}
        self._arena = self._digests = self._host_digests = self._copy_stream = self._thread = self._error = None
        self._host, self._closed = {}, False

    # -- what a cut copies -------------------------------------------------------------------------------------------------
    def _ranges(self, cut, extras):
        """[(name, device tensor)] of this cut: at most the 8 ranges of one ``lirec_snapshot``"""
        from . import ops
        model, optimizer = self.model, self.optimizer
        ranges = [('params', model.flat_params()), ('exp_avg', optimizer._m), ('exp_avg_sq', optimizer._v)]
        if cut['ema']['decay'] is not None:
            ranges.append(('ema', optimizer.ema))
        if cut['window']['phase'] != 0:
            ranges.append(('grads', model.flat_grads(attach=True)))
        if cut['guard_flags'] is not None:
            ranges.append(('skipped', optimizer._skipped_dev))
        ranges += [('extra:' + key, t.detach()) for key, t in extras.items()]
        if len(ranges) > ops.SNAPSHOT_MAX_RANGES:
            raise ValueError('AsyncCheckpointer: %d ranges, one snapshot carries %d' % (len(ranges), ops.SNAPSHOT_MAX_RANGES))
        for name, t in ranges:
            nbytes = t.numel() * t.element_size()
            if not (t.is_cuda and t.is_contiguous() and nbytes % 4 == 0 and t.data_ptr() % 16 == 0):
                raise ValueError('AsyncCheckpointer: %s (%d bytes at %#x) is no range lirec_snapshot copies: a contiguous device '
                                 'tensor of a multiple of 4 bytes on a 16-byte boundary' % (name, nbytes, t.data_ptr()))
        return ranges

    def _place(self, ranges, cut):
        """the arena's views for ``ranges``, the pinned twins and the digest words.  The arena is allocated at the first cut, with
        room for the window's gradient buffer whenever accumulate_steps > 1 (open at most cuts, closed at some), and again only
        when a later cut needs more (the average switched on in the middle of a run)"""
        up = lambda n: (n + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        sizes = [t.numel() * t.element_size() for _, t in ranges]
        need = sum(up(n) for n in sizes)
        if cut['window']['k'] > 1 and cut['window']['phase'] == 0:
            need += up(sizes[0])
        dev = ranges[0][1].device
        if self._arena is None or self._arena.numel() < need or self._arena.device != dev:
            self._arena = torch.empty(need, dtype=torch.uint8, device=dev)
        if self._digests is None or self._digests.device != dev:
            self._digests = torch.zeros(8, dtype=torch.int64, device=dev)
            self._host_digests = torch.zeros(8, dtype=torch.int64, pin_memory=True)
        if self._copy_stream is None or self._copy_stream.device != dev:
            self._copy_stream = torch.cuda.Stream(device=dev)
        views, at = [], 0
        for (name, t), n in zip(ranges, sizes):
            views.append(self._arena[at:at + n].view(t.dtype))
            at += up(n)
            h = self._host.get(name)
            if h is None or h.numel() != t.numel() or h.dtype != t.dtype:
                self._host[name] = torch.empty(t.numel(), dtype=t.dtype, pin_memory=True)
        return views

    # -- the loop's side ---------------------------------------------------------------------------------------------------
    def save(self, path, epoch, train_state=None):
        from . import ops
        t0 = time.perf_counter()
        if self._closed:
            raise RuntimeError('AsyncCheckpointer.save(): closed')
        if self._thread is not None and self._thread.is_alive():
            self.stats['waits'] += 1
        self.wait()
        if ops.CommandList.mark() >= 0:
            raise RuntimeError('AsyncCheckpointer.save(): not while a step is being recorded')
        model, optimizer = self.model, self.optimizer
        optimizer._ensure_state()
        model.join_side_streams()       # (a replayed step may still be updating bucket 0 on lane 0: what state_dict() joins)
        optimizer._join_side()
        # (everything the writer needs of model and optimiser is taken HERE, on the loop's thread: host integers, keys, shapes,
        #  offsets, metadata -- the thread looks at neither object again)
        cut = optimizer.host_cut()
        model_layout, state_layout = model.state_dict_layout(), optimizer.state_layout()
        ranges = self._ranges(cut, model_layout[2])
        views = self._place(ranges, cut)
        ops.snapshot([(t.reshape(-1), v) for (_, t), v in zip(ranges, views)], self._digests)
        taken = torch.cuda.Event()
        taken.record()
        self._copy_stream.wait_event(taken)
        with torch.cuda.stream(self._copy_stream):
            for (name, _), v in zip(ranges, views):
                self._host[name].copy_(v, non_blocking=True)
            self._host_digests.copy_(self._digests, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record()
        self._arena.record_stream(self._copy_stream)
        self._digests.record_stream(self._copy_stream)
        dir_check(os.path.dirname(path))
        job = {'path': path, 'epoch': epoch, 'train_state': train_state, 'cut': cut, 'names': [name for name, _ in ranges],
               'copied': copied, 'group_names': _group_names(optimizer), 'model_layout': model_layout, 'state_layout': state_layout,
               'offsets': dict(model._offsets)}
        import threading
        self._thread = threading.Thread(target=self._run, args=(job,), name='lirec-checkpoint-writer', daemon=False)
        self._thread.start()
        self.stats['save_s'] += time.perf_counter() - t0

    def wait(self):
        """until no write is in flight; raises what the writer raised"""
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    def close(self):
        if self._closed:
            return
        self._closed = True
        try:
            self.wait()
        finally:
            self._arena = self._digests = self._host_digests = self._copy_stream = None
            self._host = {}

    # -- the writer's side: no launch, no device read -----------------------------------------------------------------------
    def _run(self, job):
        t0 = time.perf_counter()
        try:
            job['copied'].synchronize()
            write_atomic(self._build(job), job['path'])
            self.stats['writes'] += 1
        except BaseException as e:        # (never lost: raised from the next save(), wait() or close())
            self._error = e
        finally:
            self.stats['writer_s'] += time.perf_counter() - t0

    def _build(self, job):
        import numpy as np
        host = {name: self._host[name] for name in job['names']}
        want = self._host_digests.numpy().view(np.uint64)
        for i, name in enumerate(job['names']):
            got = host[name].numpy().reshape(-1).view(np.uint32).sum(dtype=np.uint64)
            if int(got) != int(want[i]):
                raise RuntimeError('AsyncCheckpointer: the host copy of %s does not carry the digest the snapshot left on the device '
                                   '(%#x, not %#x): arena or pinned memory was reused before the copy had finished'
                                   % (name, int(got), int(want[i])))
        A = type(self.optimizer)
        cut, layout = job['cut'], job['model_layout']
        skipped = int(host['skipped'][0]) if 'skipped' in host else 0
        shapes = {key: shape for key, shape, _ in layout[0]}
        extras = {name[len('extra:'):]: h.view(shapes[name[len('extra:'):]]) for name, h in host.items() if name.startswith('extra:')}
        sd = self.model.state_dict_from(host['params'], extras, layout=layout)
        osd = self.optimizer.state_dict_from(host['exp_avg'], host['exp_avg_sq'], A.steps_at(cut, skipped), cut['param_groups'],
                                             layout=job['state_layout'])
        ema = None
        if 'ema' in host:
            ema = ema_entry_from(cut['ema']['decay'], A.ema_updates_at(cut, skipped), A.ema_state_dict_from(host['ema'], sd, job['offsets']))
        ts = job['train_state']
        if ts is not None:
            ts = dict(ts, skipped_total=A.skipped_total_at(cut, skipped),
                      window=A.window_state_from(cut['window']['phase'], cut['window']['k'], host.get('grads')))
        return checkpoint_dict(job['epoch'], sd, osd, job['group_names'], ema, ts)


def load_train_state(path_or_dict):
    """``(checkpoint dict, ck['train_state'])`` of a path or an already loaded checkpoint; a checkpoint written without
    ``opt.save_train_state`` -- the reference's three keys -- is refused in words: it does not say where the run was."""
    ck = path_or_dict
    if not isinstance(ck, dict):
        ck = torch.load(os.fspath(ck), map_location='cpu', weights_only=False)
    if 'train_state' not in ck:
        raise ValueError('this checkpoint holds no train state (keys: %s): it was written without opt.save_train_state and can '
                         'start a run, not continue one -- training(resume=) needs ck[\'train_state\']' % sorted(ck))
    return ck, ck['train_state']


def load_model(name=None, path=None, ema=False):
    """``checkpoint['state_dict']`` of ``opt.resume_str`` (utils/util_functions.py:274-281); ``ema``: the averaged weights the
    checkpoint was written with (``ck['ema']['state_dict']``: same keys and shapes) -- a KeyError when it has none."""
    ck = torch.load(path or opt.resume_str, map_location='cpu', weights_only=False)
    if ema:
        if 'ema' not in ck:
            raise KeyError('%s holds no EMA weights (it was written with ema_decay off)' % (path or opt.resume_str))
        return ck['ema']['state_dict']
    return ck['state_dict']


def load_ema(optimizer, path=None):
    """the shadow and its count from a checkpoint written with the average on; a checkpoint without ``'ema'`` leaves the optimiser
    as it is -- its shadow starts from the parameters.  Returns whether anything was loaded."""
    ck = torch.load(path or opt.resume_str, map_location='cpu', weights_only=False)
    if 'ema' not in ck:
        return False
    optimizer.load_ema_state_dict(ck['ema']['state_dict'], updates=ck['ema'].get('updates'))
    return True


def load_optimizer(path=None):
    """``checkpoint['optimizer']`` (utils/util_functions.py:283-291)."""
    ck = torch.load(path or opt.resume_str, map_location='cpu', weights_only=False)
    return ck['optimizer']


# ---------------------------------------------------------------------------
# checkpoint <-> flat buffers
# ---------------------------------------------------------------------------

def checkpoint_to_flat(ck: dict, model) -> dict:
    """Reference-layout checkpoint dict -> the hot path's flat fp32 buffers, in ``model``'s flat order
    (``model._offsets``: heads + gate | interaction embed | context embed, every tensor 16-byte aligned):
    ``{'params', 'exp_avg', 'exp_avg_sq': 1-D fp32 tensors of model._n_flat elements, 'step': int, 'epoch': int,
    'offsets': {name: (offset, numel)}}``.  This is what a host that drives the C ABI without torch modules
     uploads for ``lirec_adam_step`` and the GEMMs.  Optimizer state is optional.  ``'step'`` is the furthest
    parameter's; parameters that have received fewer updates (frozen for a while: torch.optim.Adam keeps a step per parameter)
    are listed in ``'lags'``: {name: step - its own} -- what ``lirec_adam_step_ranges`` takes per range; absent when all agree.
    PARAMETER GROUPS: an optimizer state with more than one group numbers its parameters group by group, so the names of each
    group's parameters are needed -- ``ck['param_group_names']`` ([[names of group 0], ...]: FusedAdam.group_names(), which
    ``flat_to_checkpoint`` writes too) -- and the result carries ``'groups'``: [{'lr', 'betas', 'eps', 'weight_decay', 'amsgrad',
    'names'}, ...], the rows of ``lirec_adam_step_groups``' table and who reads which (``'decoupled_weight_decay'`` among the
    keys when the state has it).  One group: no such key, as ever -- and ``'decoupled_weight_decay': True`` ONLY when the one
    group is decoupled (AdamW): the update rule is then another, and the by-value ``lirec_adam_step`` does not have it."""
    sd = ck['state_dict']
    names = [n for n, _ in model.named_parameters()]
    if list(sd.keys()) != names:
        raise ValueError('checkpoint keys do not match the model: %s' % sorted(set(sd) ^ set(names)))
    n = model._n_flat
    out = {'params': torch.zeros(n), 'exp_avg': torch.zeros(n), 'exp_avg_sq': torch.zeros(n), 'step': 0,
           'epoch': int(ck.get('epoch', 0)), 'offsets': dict(model._offsets)}
    pd = dict(model.named_parameters())
    for k in names:
        off, cnt = model._offsets[k]
        if tuple(sd[k].shape) != tuple(pd[k].shape):
            raise ValueError('shape of %s: checkpoint %s, model %s' % (k, tuple(sd[k].shape), tuple(pd[k].shape)))
        out['params'][off:off + cnt] = sd[k].reshape(-1).float()
    osd = ck.get('optimizer')
    if osd and osd.get('state'):
        # torch numbers optimizer state by position in param_groups[*]['params'] = model.parameters() order
        order = [i for g in osd['param_groups'] for i in g['params']]
        by_group = names
        if len(osd['param_groups']) > 1:
            gn = ck.get('param_group_names')
            if gn is None or [len(x) for x in gn] != [len(g['params']) for g in osd['param_groups']] or \
                    sorted(n for x in gn for n in x) != sorted(names):
                raise ValueError('an optimizer state with %d parameter groups needs ck[\'param_group_names\'] -- the parameter names '
                                 'of every group, in the groups\' order (FusedAdam.group_names())' % len(osd['param_groups']))
            by_group = [n for x in gn for n in x]
            out['groups'] = [dict({k: v for k, v in g.items() if k != 'params'}, names=list(x)) for g, x in zip(osd['param_groups'], gn)]
        elif osd['param_groups'] and osd['param_groups'][0].get('decoupled_weight_decay'):
            out['decoupled_weight_decay'] = True
        steps = {}
        for idx, k in zip(order, by_group):
            st = osd['state'].get(idx)
            if st is None:
                steps[k] = 0          # (a parameter stock Adam never updated has no state)
                continue
            off, cnt = model._offsets[k]
            out['exp_avg'][off:off + cnt] = st['exp_avg'].reshape(-1).float()
            out['exp_avg_sq'][off:off + cnt] = st['exp_avg_sq'].reshape(-1).float()
            steps[k] = int(float(st['step']))
        out['step'] = max(steps.values()) if steps else 0
        lags = {k: out['step'] - t for k, t in steps.items() if t != out['step']}
        if lags:
            out['lags'] = lags
    return out


def flat_to_checkpoint(flat: dict, model, lr=None, weight_decay=None) -> dict:
    """Inverse of ``checkpoint_to_flat``: the reference's ``{'epoch', 'state_dict', 'optimizer'}`` dict, with an
    optimizer state_dict a stock ``torch.optim.Adam`` over ``model.parameters()`` loads -- with ``flat['groups']``, one built with
    the same groups (parameters numbered group by group, and ``'param_group_names'`` beside the optimizer state)."""
    from collections import OrderedDict
    names = [n for n, _ in model.named_parameters()]
    pd = dict(model.named_parameters())
    sd, state = OrderedDict(), {}
    number = {k: i for i, k in enumerate(names)}
    if flat.get('groups'):
        number = {k: i for i, k in enumerate(n for g in flat['groups'] for n in g['names'])}
        if sorted(number) != sorted(names):
            raise ValueError('flat[\'groups\'] does not name every parameter of the model exactly once')
    for k in names:
        i = number[k]
        off, cnt = flat['offsets'][k] if 'offsets' in flat else model._offsets[k]
        shp = pd[k].shape
        sd[k] = flat['params'][off:off + cnt].clone().view(shp)
        state[i] = {'step': torch.tensor(float(flat['step'] - flat.get('lags', {}).get(k, 0))), 'exp_avg': flat['exp_avg'][off:off + cnt].clone().view(shp),
                    'exp_avg_sq': flat['exp_avg_sq'][off:off + cnt].clone().view(shp)}
    group = {'lr': opt.lr if lr is None else lr, 'betas': (0.9, 0.999), 'eps': 1e-8,
             'weight_decay': opt.weight_decay if weight_decay is None else weight_decay, 'amsgrad': False,
             'params': list(range(len(names)))}
    if flat.get('decoupled_weight_decay'):
        group['decoupled_weight_decay'] = True          # (AdamW: torch.optim.Adam's key; absent = coupled, as ever)
    if flat.get('groups'):
        groups, at = [], 0
        for g in flat['groups']:
            groups.append(dict({k: v for k, v in g.items() if k != 'names'}, params=list(range(at, at + len(g['names'])))))
            at += len(g['names'])
        return {'epoch': int(flat.get('epoch', 0)), 'state_dict': sd, 'optimizer': {'state': state, 'param_groups': groups},
                'param_group_names': [list(g['names']) for g in flat['groups']]}
    return {'epoch': int(flat.get('epoch', 0)), 'state_dict': sd, 'optimizer': {'state': state, 'param_groups': [group]}}
