"""Resident block store: a TILED dataset kept in HBM, batches drawn from it by sample id.

The recipes that run on a tiled dataset -- ``modalties``, ``int_rels``, ``int_ch``, or the reference's own ``MixedFeaturesDataset``
plugged in as INTEGRATION.md describes -- pay per batch for a float64 ``features`` block through ``default_collate``, a host-to-
device copy, a cast kernel and (training) a staging pass.  Here the feature rows of EVERY sample are stored once on the device as
q32b, the storage layer 1 and its weight gradient gather their rows from; the other fields of the samples are stacked once, in
``default_collate``'s dtypes, and uploaded once.  A batch is then a list of sample ids: one ``lirec_collate_fields`` launch copies
the field rows, and the model hands the ids to the library (``lirec_set_feature_rows``), which turns "row p of the batch's block"
into "row p % rows_per_clip of sample ids[p / rows_per_clip]" in the row lists the kernels gather through.  The features never
move again, and every value is bit-identical to the same samples collated on the host and stored as a per-batch q32b block
(``to_device_batch(default_collate(samples), feature_dtype='q32')``).

Layout contract: sample s owns storage rows [s * rows_per_clip, (s + 1) * rows_per_clip) of ONE q32b matrix of D columns
(rows_per_clip = the product of the feature's leading dims, D % 32 == 0); the matrix's rows are padded to a multiple of 32 and the
padding is zeroed once.  Every sample has the same shapes.  At most ``FEATURE_ROWS_MAX`` rows (int32 row lists), and no more bytes
than the device has free minus ``MARGIN_BYTES``.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import FEATURE_ROWS_MAX, LirecError

MARGIN_BYTES = 1 << 30           # device memory a store leaves free beyond its own bytes (activations, workspaces, the allocator's slack)
CHUNK_BYTES = 64 << 20           # host bytes of feature rows that go up in one copy while the store is filled
IDS_KEY = 'clip_ids'             # the batch's own sample ids in the batch buffer (what the forward's row mapping reads)


def _free_bytes(device) -> int:
    return int(torch.cuda.mem_get_info(torch.device(device))[0])


def _collate_fields(samples, feature_key):
    """``default_collate`` of the samples' fields other than the features: {key: tensor [len(samples), ...]} in its dtypes"""
    rest = [{k: v for k, v in s.items() if k != feature_key} for s in samples]
    try:
        out = torch.utils.data.default_collate(rest) if rest and rest[0] else {}
    except (RuntimeError, TypeError) as e:
        raise LirecError('BlockStore: the samples\' fields cannot be stacked (every sample must have the same shapes): %s' % str(e)[:160])
    for k, v in out.items():
        if not torch.is_tensor(v):
            raise LirecError('BlockStore: field %r is not numeric (%s): a resident store holds tensors only' % (k, type(v).__name__))
    return out


def batch_layout(fields, B):
    """The layout of a block-store batch's one buffer, ``[(key, offset, nbytes, dtype, shape)]`` and its size: every field of
    ``fields`` = ``[(key, numpy dtype, per-sample shape)]`` for ``B`` samples, then the batch's sample ids (int32 [B]); every entry
    at a multiple of 256 bytes.  Static: every batch of ``B`` samples of one store has it (``features.layout_views`` cuts it)."""
    layout, off = [], 0
    for k, dt, shape in list(fields) + [(IDS_KEY, np.dtype(np.int32), ())]:
        shape = (int(B),) + tuple(int(x) for x in shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
        layout.append((k, off, nbytes, np.dtype(dt), shape))
        off += (nbytes + 255) // 256 * 256
    return layout, max(off, 256)


def storage_rows(ids, rows_per_clip, phys_rows):
    """numpy statement of the row mapping (include/lirec_hip.h, lirec_feature_rows): storage row of batch-local physical rows"""
    p = np.asarray(phys_rows, dtype=np.int64)
    return np.asarray(ids, dtype=np.int64)[p // rows_per_clip] * rows_per_clip + p % rows_per_clip


class BlockStore:
    """The samples of ``dataset_or_samples`` (a map-style dataset or a sequence of sample dicts) resident on ``device``.
    ``n``, ``rows_per_clip``, ``feature_shape`` (per sample), ``D``, ``store_rows``, ``nbytes`` (features + fields), ``fields``
    (``[(key, numpy dtype, per-sample shape)]``, the samples' key order) and ``keys`` (all keys, the features in their place).
    ``capacity``: sample slots (>= the samples given; the rest is filled by ``update``).  ``upload=False``: the plan only -- every
    check, no device memory (what a host without a GPU can ask: ``BlockLoader.layout``).
    Refuses (LirecError, before any device memory is taken where the first chunk shows it): ragged feature shapes, D % 32 != 0,
    non-numeric fields, capacity * rows_per_clip >= the row limit, a store larger than the free device memory minus
    ``MARGIN_BYTES``."""

    def __init__(self, dataset_or_samples, device, feature_key='features', capacity=None, upload=True):
        src, n_src = dataset_or_samples, len(dataset_or_samples)
        self.feature_key, self.device = feature_key, torch.device(device)
        self.n = int(n_src if capacity is None else capacity)
        if n_src < 1 or self.n < n_src:
            raise LirecError('BlockStore: %d samples for %d slots' % (n_src, self.n))
        first = src[0]
        if not isinstance(first, dict) or feature_key not in first:
            raise LirecError('BlockStore: samples must be dicts with %r' % feature_key)
        f0 = np.asarray(first[feature_key])
        if f0.ndim < 1 or f0.dtype not in (np.float32, np.float64):
            raise LirecError('BlockStore: %r must be a float32 / float64 array (..., D), not %s %s' % (feature_key, f0.dtype, f0.shape))
        self.feature_shape, self.D = tuple(int(x) for x in f0.shape), int(f0.shape[-1])
        self.rows_per_clip = int(np.prod(f0.shape[:-1], dtype=np.int64))
        if self.D % 32 != 0 or self.D < 32:
            raise LirecError('BlockStore: the feature width %d is not a multiple of 32 (q32b storage)' % self.D)
        if self.rows_per_clip < 1 or self.n * self.rows_per_clip >= FEATURE_ROWS_MAX:
            raise LirecError('BlockStore: %d samples x %d rows reach the row limit of a q32b store (%d: its row lists are int32)'
                             % (self.n, self.rows_per_clip, FEATURE_ROWS_MAX))
        one = _collate_fields([first], feature_key)
        self.fields = [(k, np.dtype(torch.empty(0, dtype=v.dtype).numpy().dtype), tuple(v.shape[1:])) for k, v in one.items()]
        self.keys = [k for k in first]
        self.store_rows = (self.n * self.rows_per_clip + 31) // 32 * 32
        field_bytes = sum(int(np.prod(sh, dtype=np.int64)) * dt.itemsize for _, dt, sh in self.fields) * self.n + 4 * self.n
        self.nbytes = self.store_rows * self.D * 4 + field_bytes
        self.data = self.tables = None
        # the first chunk on the host: what it shows (ragged shapes, fields that do not stack) is refused before any device memory
        per = max(1, CHUNK_BYTES // max(f0.nbytes, 1))
        chunk0 = [first] + [src[i] for i in range(1, min(per, n_src))]
        feats0 = self._stack_features(chunk0, 0)
        fields0 = _collate_fields(chunk0, feature_key)
        if not upload:
            return
        if self.device.type != 'cuda':
            raise LirecError('BlockStore: a resident store lives on a GPU (device %s): there is no CPU path' % self.device)
        free = _free_bytes(self.device)
        if self.nbytes > free - MARGIN_BYTES:
            raise LirecError('BlockStore: the store needs %d bytes, the device has %d free and %d of them stay free (MARGIN_BYTES)'
                             % (self.nbytes, free, MARGIN_BYTES))
        from . import ops
        self.data = torch.empty(max(self.store_rows * self.D * 4, 256), dtype=torch.uint8, device=self.device)
        if self.data.data_ptr() % 256 != 0:
            raise LirecError('BlockStore: the allocator returned storage that is not 256-byte aligned')
        used = self.n * self.rows_per_clip
        if self.store_rows > used:        # the rows up to the multiple of 32: zeroed once (no sample ever owns them)
            ops.q32b_write_rows(torch.zeros(self.store_rows - used, self.D, dtype=torch.float32, device=self.device), self.data, used,
                                self.store_rows)
        self.tables = {k: torch.zeros((self.n,) + sh, dtype=torch.from_numpy(np.zeros(0, dtype=dt)).dtype, device=self.device)
                       for k, dt, sh in self.fields}
        self.tables[IDS_KEY] = torch.arange(self.n, dtype=torch.int32, device=self.device)
        at, chunk, feats, fields = 0, chunk0, feats0, fields0
        while True:
            self._write(at, feats, fields)
            at += len(chunk)
            if at >= n_src:
                break
            chunk = [src[i] for i in range(at, min(at + per, n_src))]
            feats, fields = self._stack_features(chunk, at), _collate_fields(chunk, feature_key)

    def _stack_features(self, samples, at):
        arrs = [np.asarray(s[self.feature_key]) for s in samples]
        for j, a in enumerate(arrs):
            if tuple(a.shape) != self.feature_shape:
                raise LirecError('BlockStore: ragged features -- sample %d is %s, sample 0 is %s (a store holds one shape)'
                                 % (at + j, tuple(a.shape), self.feature_shape))
        return torch.from_numpy(np.ascontiguousarray(np.stack(arrs)))

    def _write(self, at, feats, fields):
        from . import ops
        ops.q32b_write_rows(feats.to(self.device).contiguous(), self.data, at * self.rows_per_clip, self.store_rows)
        if set(fields) != {k for k, _, _ in self.fields}:
            raise LirecError('BlockStore: samples with different fields (%s against %s)' % (sorted(fields), sorted(k for k, _, _ in self.fields)))
        for k, v in fields.items():
            dst = self.tables[k]
            if v.dtype != dst.dtype or tuple(v.shape[1:]) != tuple(dst.shape[1:]):
                raise LirecError('BlockStore: field %r changes dtype or shape between samples' % k)
            dst[at:at + v.shape[0]].copy_(v)

    def update(self, ids, features, fields=None):
        """Overwrite the feature rows of samples ``ids`` with ``features`` ((len(ids), *feature_shape), float32 / float64, host or
        device) -- converted as the store was filled, on the current stream -- and, with ``fields`` ({key: [len(ids), ...]}), their
        field rows."""
        from . import ops
        ids = [int(i) for i in ids]
        if any(i < 0 or i >= self.n for i in ids):
            raise IndexError('BlockStore.update: a sample id outside [0, %d)' % self.n)
        f = torch.as_tensor(features)
        if tuple(f.shape) != (len(ids),) + self.feature_shape or f.dtype not in (torch.float32, torch.float64):
            raise LirecError('BlockStore.update: features must be %s float32 / float64' % ((len(ids),) + self.feature_shape,))
        f = f.to(self.device).contiguous()
        for j, i in enumerate(ids):
            ops.q32b_write_rows(f[j], self.data, i * self.rows_per_clip, self.store_rows)
        for k, v in (fields or {}).items():
            dst = self.tables[k]
            dst[torch.as_tensor(ids, device=self.device)] = torch.as_tensor(v).to(device=self.device, dtype=dst.dtype)

    def set_field(self, key, values):
        """one more stacked field ([n, ...] tensor or array; e.g. per-clip loss weights): it rides in every batch from now on"""
        v = torch.as_tensor(values)
        if v.shape[0] != self.n:
            raise LirecError('BlockStore.set_field: %d rows for %d samples' % (v.shape[0], self.n))
        self.fields = [f for f in self.fields if f[0] != key] + [(key, np.dtype(torch.empty(0, dtype=v.dtype).numpy().dtype), tuple(v.shape[1:]))]
        if key not in self.keys:
            self.keys.append(key)
        if self.tables is not None:
            self.tables[key] = v.to(self.device).contiguous()

    def features_of(self, clip_ids, B=None):
        """the feature block of the batch ``clip_ids`` (int32 device tensor [B]): a ``Q32Block`` over the whole store, no copy"""
        from . import ops
        B = clip_ids.numel() if B is None else B
        return ops.Q32Block(self.data, (B,) + self.feature_shape, clip_ids=clip_ids, rows_per_clip=self.rows_per_clip,
                            store_rows=self.store_rows)


class ResidentBlockDataset(torch.utils.data.Dataset):
    """A tiled dataset with its samples resident on ``device`` (None: ``opt.device``): ``training()`` / ``testing()`` /
    ``predict()`` then draw it with ``lirec_amd.loader.BlockLoader``.  ``__getitem__`` still returns the host sample; what the
    loops read of the dataset (``n_classes``, ``n_rels``, ``rels_list``, ``interidx2mgdidx``, ...) reads through, ``epoch`` is
    passed on."""

    def __init__(self, dataset, device=None, feature_key='features'):
        from .config import opt
        if getattr(dataset, 'context_draw', 'strided') == 'random':
            # (the store would freeze whichever epoch's draw it was filled from; BlockStore.update is the way to change its samples)
            raise LirecError('ResidentBlockDataset: a dataset with context_draw=\'random\' redraws its context every epoch, a block store '
                             'holds one copy of every sample: make the store from a \'strided\' dataset')
        self.dataset = dataset
        self.block_store = BlockStore(dataset, opt.device if device is None else device, feature_key)
        self._weights = None

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        s = self.dataset[idx]
        if self._weights is not None:
            from .features import CLIP_WEIGHT
            s = dict(s)
            s[CLIP_WEIGHT] = np.float64(self._weights[idx])
        return s

    def __getattr__(self, name):                 # (only reached for what the wrapper itself does not have)
        if name in ('dataset', 'block_store', '_weights'):
            raise AttributeError(name)
        return getattr(self.dataset, name)

    @property
    def epoch(self):
        return getattr(self.dataset, 'epoch', 0)

    @epoch.setter
    def epoch(self, value):
        self.dataset.epoch = value

    @property
    def carries_clip_weights(self):
        return self._weights is not None or getattr(self.dataset, 'carries_clip_weights', False)

    def set_clip_weights(self, weights):
        """per-clip loss weights (``lirec_amd.data.with_clip_weights``): one more field of the store, ``clip_weight`` [n] float64"""
        from .features import CLIP_WEIGHT, checked_clip_weights
        self._weights = checked_clip_weights(weights, len(self))
        self.block_store.set_field(CLIP_WEIGHT, torch.from_numpy(self._weights.copy()))

    def update(self, ids, features):
        self.block_store.update(ids, features)

    def device_tables(self, device=None):
        """the stacked fields on the device, {key: [n, ...]} (+ the id table): uploaded once, when the store was built"""
        st = self.block_store
        if device is not None and torch.device(device).type != st.device.type:
            raise LirecError('the block store lives on %s' % st.device)
        return st.tables
