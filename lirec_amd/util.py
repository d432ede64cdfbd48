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
    return {'decay': float(optimizer.ema_decay), 'updates': int(optimizer.ema_updates()), 'state_dict': optimizer.ema_state_dict()}


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
        ck = {'epoch': epoch, 'state_dict': model.state_dict(), 'optimizer': optimizer.state_dict()}
        if len(getattr(optimizer, 'param_groups', ())) > 1 and hasattr(optimizer, 'group_names'):
            ck['param_group_names'] = optimizer.group_names()       # (who is in which group: checkpoint_to_flat needs it)
        ema = ema_entry(optimizer)
        if ema is not None:
            ck['ema'] = ema                 # (beside the optimizer state, which stays what a stock Adam loads)
        if train_state is not None:
            ck['train_state'] = train_state
        if atomic:
            tmp = '%s.tmp.%d' % (path, os.getpid())
            try:
                torch.save(ck, tmp)
                os.replace(tmp, path)
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
        else:
            torch.save(ck, path)
    if multi:
        dist.barrier()


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
