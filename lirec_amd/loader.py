"""Batch loader on THREADS for datasets whose per-batch work is a ``collate_fn`` of GIL-free array copies
(lirec_amd.features.PiecesDataset): the ``torch.utils.data.DataLoader`` protocol ``training()`` / ``testing()`` use
(mlp/train.py:33-37, mlp/test.py:18-22 -- dataset, batch_size, shuffle / sampler, num_workers, drop_last; ``len()``; one
pass per ``iter()``), with ``num_workers`` threads instead of worker processes.

Why not worker processes here: they are forked from a process that has initialised the GPU, and with eight of them alive
the same train step took 36 ms of GPU time instead of 1 ms on the MI355X box (profiles/r03_training_entry.txt); a batch of
piece tables is also 2.4 MB that would cross a pipe and be pinned again on the other side.  Threads hand over the pinned
tensors the collate wrote.  Batches come out in sampler order whatever the thread count."""
from __future__ import annotations

import queue
import threading

import torch


class ThreadedLoader:
    def __init__(self, dataset, batch_size=1, shuffle=False, sampler=None, num_workers=0, collate_fn=None, drop_last=False,
                 prefetch=4):
        self.dataset, self.collate_fn = dataset, collate_fn or torch.utils.data.default_collate
        if sampler is None:
            sampler = torch.utils.data.RandomSampler(dataset) if shuffle else torch.utils.data.SequentialSampler(dataset)
        self.batch_sampler = torch.utils.data.BatchSampler(sampler, batch_size, drop_last)
        self.num_workers, self.prefetch = max(int(num_workers), 0), max(int(prefetch), 1)

    def __len__(self):
        return len(self.batch_sampler)

    def _make(self, idx):
        return self.collate_fn([self.dataset[i] for i in idx])

    def __iter__(self):
        return self._batches(None)

    def iter_from(self, start):
        """an epoch's batches from the ``start``-th on (a resumed run, lirec_amd.train): the batch sampler is drawn HERE, whole --
        the permutation comes from the caller's RNG state as it is at this call -- and no sample of the batches passed over is
        fetched"""
        return self._batches(list(self.batch_sampler)[int(start):])

    def _batches(self, todo):
        if self.num_workers == 0:
            for idx in (self.batch_sampler if todo is None else todo):
                yield self._make(idx)
            return
        if todo is None:
            todo = list(self.batch_sampler)                 # (the sampler is drawn on the caller's thread: its RNG state is the caller's)
        n, depth = len(todo), self.num_workers * self.prefetch
        slots = [queue.Queue(maxsize=1) for _ in range(n)]  # one slot per batch: ordered hand-over
        nxt, lock, stop = [0], threading.Lock(), threading.Event()
        room = threading.Semaphore(depth)                   # at most `depth` batches built ahead of the consumer

        def work():
            while not stop.is_set():
                room.acquire()
                with lock:
                    k = nxt[0]
                    nxt[0] += 1
                if k >= n or stop.is_set():
                    return
                try:
                    slots[k].put(('ok', self._make(todo[k])))
                except BaseException as e:                  # handed to the consumer, which re-raises it in order
                    slots[k].put(('err', e))
        threads = [threading.Thread(target=work, daemon=True) for _ in range(self.num_workers)]
        for t in threads:
            t.start()
        try:
            for k in range(n):
                kind, val = slots[k].get()
                slots[k] = None
                room.release()
                if kind == 'err':
                    raise val
                yield val
        finally:
            stop.set()
            for _ in threads:
                room.release()


def device_collate_in_force(dataset, device=None) -> bool:
    """``opt.device_collate`` asks for ``ResidentLoader``; it is used when the dataset keeps its pieces in a resident store, the
    device is a GPU and the gathered q32b path is in force (what a recorded train step asks for, lirec_amd.train._recordable).
    Anything else keeps ``ThreadedLoader`` -- a dataset that carries per-clip loss weights too: ``lirec_collate_resident`` gathers
    the nine fields, not the weights."""
    from .config import opt
    from .features import CLIP_WEIGHT
    device = opt.device if device is None else device
    if CLIP_WEIGHT in (getattr(dataset, '_stacked', None) or ()) or getattr(dataset, 'carries_clip_weights', False):
        return False
    return bool(getattr(opt, 'device_collate', False)) and getattr(dataset, 'store', None) is not None and \
        getattr(dataset, 'emit', None) == 'pieces' and hasattr(dataset, 'device_tables') and str(device).startswith('cuda') and \
        bool(getattr(opt, 'pieces_gather', True)) and bool(getattr(opt, 'pieces_q32b', False)) and bool(getattr(opt, 'layer1_planes', False))


def block_store_in_force(dataset, device=None) -> bool:
    """``BlockLoader`` draws ``dataset`` when it keeps its samples in a resident block store (lirec_amd.blockstore) and the device is
    a GPU.  (Nothing else is asked: a model that cannot read such batches -- ``opt.layer1_planes`` off, another GEMM core -- says so
    itself, there is no other path to fall back to.)  A wrapper that adds per-clip weights AROUND the store would lose them --
    the store's batches carry the store's fields -- and is refused."""
    from .config import opt
    from .features import CLIP_WEIGHT
    from ._lib import LirecError
    store = getattr(dataset, 'block_store', None)
    device = opt.device if device is None else device
    if store is None or store.tables is None or not str(device).startswith('cuda'):
        return False
    if getattr(dataset, 'carries_clip_weights', False) and CLIP_WEIGHT not in store.keys:
        raise LirecError('per-clip weights wrapped around a resident block store do not reach its batches: give them to the store '
                         '(ResidentBlockDataset.set_clip_weights / data.with_clip_weights) or wrap the dataset before it is made resident')
    return True


def make_loader(dataset, batch_size, shuffle=False, sampler=None):
    """What ``training()``, ``testing()`` and ``predict()`` draw ``dataset`` with: ``ResidentLoader`` where ``device_collate_in_force``
    (the batch buffer written on the device), ``BlockLoader`` for a tiled dataset resident in a block store (``block_store_in_force``),
    ``ThreadedLoader`` for a dataset that brings its own ``collate_fn`` (PiecesDataset: piece tables + index, built on
    ``opt.num_workers`` threads), else the stock ``DataLoader`` (mlp/train.py:33-37, mlp/test.py:18-22)."""
    from .config import opt
    kw = dict(batch_size=batch_size, shuffle=shuffle, sampler=sampler, drop_last=False)
    if block_store_in_force(dataset):
        return BlockLoader(dataset, device=opt.device, **kw)
    if device_collate_in_force(dataset):
        return ResidentLoader(dataset, device=opt.device, **kw)
    if getattr(dataset, 'collate_fn', None) is not None:
        return ThreadedLoader(dataset, num_workers=opt.num_workers, collate_fn=dataset.collate_fn, **kw)
    return torch.utils.data.DataLoader(dataset, num_workers=opt.num_workers, **kw)


class ResidentLoader:
    """Batches of a ``PiecesDataset(resident=True, emit='pieces')`` collated ON THE DEVICE: the stacked sample tables are uploaded
    once (``PiecesDataset.device_tables``), an epoch's sample ids go up in one copy, and every ``next()`` is one
    ``ops.collate_resident`` on the current stream -- no loader thread, no pinned staging buffer, no per-batch host-to-device copy,
    no host read.  A batch has the keys, dtypes, shapes and values of ``batch_to_device(dataset.collate_fn(samples))`` -- device
    views of one buffer, ``piece_store``, ``_layout``, ``_dev_blob`` -- without ``_blob`` / ``_slots`` / ``piece_counts`` (the row
    lists' padding names the store's zero row, so their whole length may be used).  The batch sampler is drawn on the caller's
    thread, all at once, exactly as ``ThreadedLoader`` with workers draws it: the same torch seed gives the same batches.

    ``bind(layout, blob)``: from now on a batch of that layout is written straight into ``blob`` (the input buffer of a recorded
    train step) instead of a buffer of its own; the call is stream-ordered behind whatever was enqueued before ``next()``, i.e.
    behind the previous replay.  ``unbind()`` ends it.  ``n_collate`` / ``n_in_place`` count the collate calls and those that wrote
    into the bound buffer.  The workspace belongs to the loader: its batches must be drawn on one stream.

    Over a ``PiecesDataset(context_draw='random')`` every ``iter()`` first brings the resident index to the draw of
    ``dataset.epoch`` (``draw_context``: one launch per epoch, none when the table already holds that epoch); ``collate_ids``
    called on its own reads the table as it is."""

    def __init__(self, dataset, batch_size=1, shuffle=False, sampler=None, drop_last=False, device='cuda'):
        if getattr(dataset, 'store', None) is None or getattr(dataset, 'emit', None) != 'pieces':
            raise ValueError('ResidentLoader needs a PiecesDataset(resident=True, emit=\'pieces\')')
        self.dataset, self.device = dataset, torch.device(device)
        if sampler is None:
            sampler = torch.utils.data.RandomSampler(dataset) if shuffle else torch.utils.data.SequentialSampler(dataset)
        self.batch_sampler = torch.utils.data.BatchSampler(sampler, batch_size, drop_last)
        self.n_collate = self.n_in_place = self.n_draw = 0
        self._bound = None                  # (layout, blob)
        self._layouts = {}                  # batch size -> (layout, nbytes)
        self._tabs = self._ws = self._counts = None

    def __len__(self):
        return len(self.batch_sampler)

    def bind(self, layout, blob):
        self._bound = (tuple(layout), blob)

    def unbind(self):
        self._bound = None

    def layout(self, B):
        """(layout, bytes) of a batch of ``B`` samples: ``features.batch_layout``, the static form"""
        if B not in self._layouts:
            from .features import _FIELDS, batch_layout
            st = self.dataset._stacked
            fields = [(k, st[k].dtype, (B,) + tuple(st[k].shape[1:])) for k in _FIELDS]
            world = self.dataset.world
            clip_all, track_all, _ = world.piece_matrices()
            self._layouts[B] = batch_layout((B,) + tuple(st['index_rows'].shape[1:]), fields,
                                            n_all=(clip_all.shape[0], track_all.shape[0]))
        return self._layouts[B]

    def epoch_ids(self):
        """the epoch's batches as lists of sample ids: the batch sampler drawn once, on the caller's thread"""
        return [list(idx) for idx in self.batch_sampler]

    def collate_ids(self, ids, B):
        """one batch from ``B`` sample ids on the device (int32; validated by the caller)"""
        from . import ops
        from .features import _FIELDS, layout_views
        if self._tabs is None:
            self._tabs = self.dataset.device_tables(self.device)
            self._ws = ops.collate_workspace(*self._tabs['n_all'], self.device)
            self._counts = torch.empty(2, dtype=torch.int32, device=self.device)
        layout, nbytes = self.layout(B)
        in_place = self._bound is not None and self._bound[0] == tuple(layout)
        blob = self._bound[1] if in_place else torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        out = layout_views(blob, layout)
        tabs = self._tabs
        ops.collate_resident(ids, tabs['index_rows'], tabs['n_all'][0], tabs['n_all'][1], out['feature_index'], out['clip_rows'],
                             out['track_rows'], self._counts, [(tabs[k], out[k]) for k in _FIELDS], self._ws)
        self.n_collate += 1
        self.n_in_place += int(in_place)
        out['piece_store'], out['_layout'], out['_dev_blob'] = self.dataset.store, layout, blob
        return out

    def __iter__(self):
        return self._batches(None, 0)

    def iter_from(self, start):
        """an epoch's batches from the ``start``-th on (a resumed run, lirec_amd.train): the batch sampler is drawn HERE, whole, and
        no batch passed over is collated"""
        return self._batches(self.epoch_ids(), int(start))

    def _batches(self, todo, start):
        import numpy as np
        if todo is None:
            todo = self.epoch_ids()
        flat = np.fromiter((i for idx in todo for i in idx), dtype=np.int64)
        if flat.size and (int(flat.min()) < 0 or int(flat.max()) >= len(self.dataset)):
            raise IndexError('ResidentLoader: the sampler drew a sample id outside [0, %d)' % len(self.dataset))
        ids = torch.from_numpy(flat.astype(np.int32)).to(self.device)         # the epoch's order: one host-to-device copy
        self.draw_context()
        at = sum(len(idx) for idx in todo[:start])
        for idx in todo[start:]:
            B = len(idx)
            yield self.collate_ids(ids[at:at + B], B)
            at += B

    def draw_context(self):
        """``PiecesDataset(context_draw='random')``: the resident index holds the draw of ``dataset.epoch`` from here on -- one
        ``ops.draw_context`` on the current stream when it holds another epoch's (``n_draw`` counts them), behind the previous
        epoch's collate calls and ahead of this epoch's.  The table belongs to the dataset: every loader over it sees the same."""
        if getattr(self.dataset, 'context_draw', 'strided') != 'random':
            return
        from . import ops
        tabs, epoch = self.dataset.device_tables(self.device), int(self.dataset.epoch)
        if tabs['drawn_epoch'] != epoch:
            ops.draw_context(tabs['slot_dst'], tabs['slot_off'], tabs['pool_rows'], tabs['index_rows'], self.dataset.R,
                             self.dataset.context_seed, epoch)
            tabs['drawn_epoch'] = epoch
            self.n_draw += 1


class _Cursor:
    """The int64 device word an in-list draw reads (``lirec_collate_fields_at``) and the host's account of it: ``at`` is the value
    the word has once everything enqueued so far has run (None: not known).  One owner, three moves: ``expect(at)`` -- the next
    draw must find ``at``: one small fill on the current stream unless the word already holds it --, ``advanced(B)`` -- a launch that
    moves the word on by ``B`` was enqueued (or will run before the next ``expect``) --, ``invalidate()``."""

    def __init__(self, device):
        self.word, self.at, self.device = None, None, device

    def expect(self, at):
        if self.word is None:
            self.word = torch.empty(1, dtype=torch.int64, device=self.device)
        if self.at != int(at):
            self.word.fill_(int(at))
            self.at = int(at)

    def advanced(self, B):
        assert self.at is not None, 'expect() first'
        self.at += int(B)

    def invalidate(self):
        self.at = None


class BlockLoader:
    """Batches of a dataset resident in a block store (``lirec_amd.blockstore.ResidentBlockDataset``), made ON THE DEVICE from
    sample ids -- ``ResidentLoader``'s contract for tiled datasets.  The batch sampler is drawn on the caller's thread, all at once
    (the same torch seed gives the same batches as the stock ``DataLoader``); the epoch's ids go up in one copy and are validated on
    the host; every ``next()`` is ONE ``ops.collate_fields`` launch on the current stream into one buffer of a static layout.  A
    batch is ``to_device_batch(default_collate([dataset[i] for i in ids]), feature_dtype='q32')`` key for key, dtype for dtype,
    value for value -- ``features`` a ``Q32Block`` over the whole store that names the batch's samples, no row copied -- plus
    ``_layout`` and ``_dev_blob``.  Duplicate ids (a sampler that draws with replacement) are fine.
    ``bind`` / ``unbind`` / ``n_collate`` / ``n_in_place`` as ``ResidentLoader``.

    ``bind(layout, blob, in_list=True)``: whoever bound the buffer draws the batch itself -- a recorded train step whose list
    begins with ``collate_at(layout, blob)``, i.e. ``lirec_collate_fields_at`` at the loader's device ``cursor`` and the launch
    that moves the cursor on by the batch.  ``next()`` then yields the views of ``blob`` WITHOUT a launch (``n_in_list`` counts
    these; ``n_collate`` does not move) and promises that the cursor names this batch when the list runs: the host keeps the value
    the device word will have (``_Cursor``) and writes the word -- one small write on the current stream -- whenever a batch
    was handed out another way in between (an epoch's start, the eager interludes).  A batch yielded so holds its values only
    once the list has run; ``materialise(batch)`` collates it after all (the step was not replayed).
    ``stable_ids`` (set by whoever will bind in-list, before the epoch is drawn): the epoch's ids go into ONE buffer of a stable
    address (``ids_base``, made once for the dataset's length, refilled by one copy per epoch) -- the address a recorded list
    holds; two live iterators of one loader would then share it, so only one may be alive.  Off (the default): every ``iter()``
    has a tensor of its own."""

    def __init__(self, dataset, batch_size=1, shuffle=False, sampler=None, drop_last=False, device='cuda'):
        if getattr(dataset, 'block_store', None) is None:
            raise ValueError('BlockLoader needs a dataset with a block_store (lirec_amd.blockstore.ResidentBlockDataset)')
        self.dataset, self.device, self.store = dataset, torch.device(device), dataset.block_store
        if sampler is None:
            sampler = torch.utils.data.RandomSampler(dataset) if shuffle else torch.utils.data.SequentialSampler(dataset)
        self.batch_sampler = torch.utils.data.BatchSampler(sampler, batch_size, drop_last)
        self.n_collate = self.n_in_place = self.n_in_list = 0
        self._bound = None                  # (layout, blob, in_list)
        self._bound_out = None              # the bound buffer's batch dict, cut once
        self._layouts = {}                  # batch size -> (layout, nbytes)
        self.stable_ids = False             # the epoch's ids in one reused buffer (what an in-list draw reads) or a tensor per epoch
        self.ids_base = None                # the epoch's ids under ``stable_ids`` (int32)
        self._cursor = _Cursor(self.device)
        self._last = None                   # the batch handed out last: (offset in the epoch's ids, B, in_list)

    def __len__(self):
        return len(self.batch_sampler)

    def bind(self, layout, blob, in_list=False):
        new = (tuple(layout), blob, bool(in_list))
        if self._bound is None or self._bound[0] != new[0] or self._bound[1] is not blob:
            self._bound_out = None
        self._bound = new

    def unbind(self):
        self._bound = self._bound_out = None

    def layout(self, B):
        """(layout, bytes) of a batch of ``B`` samples: ``blockstore.batch_layout`` of the store's fields"""
        if B not in self._layouts:
            from .blockstore import batch_layout
            self._layouts[B] = batch_layout(self.store.fields, B)
        return self._layouts[B]

    def epoch_ids(self):
        return [list(idx) for idx in self.batch_sampler]

    def _batch_of(self, layout, blob, B):
        """(the batch dict over ``blob``, the (table, view) pairs a collate launch copies -- the ids last)"""
        from .blockstore import IDS_KEY
        from .features import layout_views
        store = self.store
        views = layout_views(blob, layout)
        pairs = [(store.tables[k], views[k]) for k, _, _, _, _ in layout]
        clip_ids = views.pop(IDS_KEY)
        out = {}
        for k in store.keys:
            out[k] = store.features_of(clip_ids, B) if k == store.feature_key else views[k]
        out['_layout'], out['_dev_blob'] = layout, blob
        return out, pairs

    def collate_ids(self, ids, B):
        """one batch from ``B`` sample ids on the device (int32; validated by the caller)"""
        from . import ops
        from ._lib import COLLATE_MAX_FIELDS
        layout, nbytes = self.layout(B)
        in_place = self._bound is not None and self._bound[0] == tuple(layout)
        blob = self._bound[1] if in_place else torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        out, pairs = self._batch_of(layout, blob, B)
        for at in range(0, len(pairs), COLLATE_MAX_FIELDS):            # (one launch for up to sixteen fields: every recipe's)
            ops.collate_fields(ids, pairs[at:at + COLLATE_MAX_FIELDS])
        self.n_collate += 1
        self.n_in_place += int(in_place)
        return out

    def collate_at(self, layout, blob):
        """The launches that draw the batch at the device cursor into ``blob`` (a buffer of ``layout``) and move the cursor on by
        the batch, on the current stream: what a recorded train step puts at the head of its list (``bind(..., in_list=True)``)."""
        from . import ops
        from ._lib import COLLATE_MAX_FIELDS
        B = int(layout[-1][4][0])
        assert self.ids_base is not None and self._cursor.at is not None, 'stable_ids and cursor_to_last() first'
        _, pairs = self._batch_of(layout, blob, B)
        for at in range(0, len(pairs), COLLATE_MAX_FIELDS):
            ops.collate_fields_at(self.ids_base, self._cursor.word, B, pairs[at:at + COLLATE_MAX_FIELDS])
        ops.counter_add(self._cursor.word, [B])
        self._cursor.advanced(B)

    @property
    def cursor(self):
        """the int64 device word of the in-list draw (None before the first in-list use)"""
        return self._cursor.word

    @property
    def last_in_list(self) -> bool:
        """was the batch handed out last left for a list to draw (it holds its values only once that list has run)?"""
        return self._last is not None and self._last[2]

    def can_draw_last_in_list(self) -> bool:
        """may a list be recorded that draws the batch handed out last (its ids sit in the stable buffer)?"""
        return self.stable_ids and self._last is not None and self.ids_base is not None

    def cursor_to_last(self):
        """the device cursor names the batch handed out last: what a list that is about to be recorded on that batch draws again"""
        self._cursor.expect(self._last[0])

    def cursor_lost(self):
        """a recording that drew in-list did not finish: the word may or may not have moved -- it is written again before the next
        in-list batch"""
        self._cursor.invalidate()

    def _in_list(self, at, B):
        """the bound buffer's batch, drawn by the list that owns the buffer when it runs: no launch here"""
        self._cursor.expect(at)
        self._cursor.advanced(B)            # (what the list leaves behind)
        if self._bound_out is None:
            self._bound_out = self._batch_of(self._bound[0], self._bound[1], B)[0]
        self.n_in_list += 1
        return dict(self._bound_out)

    def materialise(self, batch):
        """the batch handed out last, collated now into a buffer of its own -- for a batch yielded in-list whose list did not run
        (its buffer still holds the previous batch); the cursor is written again before the next in-list batch"""
        at, B, in_list = self._last
        if not in_list:
            return batch
        self._cursor.invalidate()
        bound = self._bound
        self.unbind()
        try:
            out = self.collate_ids(self.ids_base[at:at + B], B)
        finally:
            self._bound = bound
        self._last = (at, B, False)
        return out

    def _upload(self, flat):
        """the epoch's ids into ``ids_base``: one host-to-device copy; the buffer is made once, for the dataset's length, and kept"""
        import numpy as np
        from ._lib import LirecError
        n = int(flat.size)
        if self.ids_base is None or self.ids_base.numel() < n:
            if self._bound is not None and self._bound[2]:
                raise LirecError('BlockLoader: an epoch of %d ids does not fit the id buffer a recorded step reads (%d)'
                                 % (n, self.ids_base.numel()))
            self.ids_base = torch.empty(max(n, len(self.dataset), 1), dtype=torch.int32, device=self.device)
        if n:
            self.ids_base[:n].copy_(torch.from_numpy(flat.astype(np.int32)))
        return self.ids_base[:n]

    def __iter__(self):
        return self._batches(None, 0)

    def iter_from(self, start):
        """an epoch's batches from the ``start``-th on (a resumed run, lirec_amd.train): the batch sampler is drawn HERE, whole; the
        epoch's ids go up as ever and the first batch handed out sits at its own offset in them -- where an in-list draw's cursor is
        then expected (``_Cursor.expect``) --; no batch passed over is collated"""
        return self._batches(self.epoch_ids(), int(start))

    def _batches(self, todo, start):
        import numpy as np
        if todo is None:
            todo = self.epoch_ids()
        flat = np.fromiter((i for idx in todo for i in idx), dtype=np.int64)
        if flat.size and (int(flat.min()) < 0 or int(flat.max()) >= self.store.n):
            raise IndexError('BlockLoader: the sampler drew a sample id outside [0, %d)' % self.store.n)
        # the epoch's order: one host-to-device copy
        ids = self._upload(flat) if self.stable_ids else torch.from_numpy(flat.astype(np.int32)).to(self.device)
        at = sum(len(idx) for idx in todo[:start])
        for idx in todo[start:]:
            B = len(idx)
            b = self._bound
            in_list = self.stable_ids and b is not None and b[2] and B > 0 and b[0] == tuple(self.layout(B)[0])
            self._last = (at, B, in_list)
            yield self._in_list(at, B) if in_list else self.collate_ids(ids[at:at + B], B)
            at += B
