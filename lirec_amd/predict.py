"""Inference -- the third entry point next to ``training`` and ``testing``: the answer for every clip of a dataset.

``predict(dataset, model, top_k=5, batch_size=None)`` runs the model over the dataset with the loader selection and the
per-recipe routing of ``lirec_amd.test.testing`` and decides every clip ON THE GPU (``lirec_predict_clips``,
include/lirec_hip.h): the joint (track, class[, relationship]) prediction of the evaluation counters, its score, the per-track
scores and the top-``top_k`` classes / relationships of the predicted track with their probabilities.  No label is read:
``labels``, ``rels_label``, ``gt_tracks`` and ``just_zeros`` may be absent from the batches.  Singleton batches are not skipped
(there is no batch statistic in ``model.eval()``).  The outputs are written into device arrays sized for the dataset; nothing
is copied back inside the loop, and each field crosses to the host once at the end.

Per recipe: the max-over-tracks recipes (``tr_maximize``) pass every clip's T candidate rows and its ``mem_mask``; ``modalties``
and ``int_rels`` use the clip-level form (T = 1, no mask) -- ``int_rels`` on row 0 of each clip's group of interaction rows, with
the clip's relationship logits.  For ``rels_multitask`` without ``tr_maximize``, when the batches carry ``hash_rel``, the
per-pair relationship scores of ``RelationshipsAcc.update`` are formed too (``Predictions.pairs``): the float32 sigmoids of the
clips of one character pair (``hash_rel != -1``), added in clip order on the host from ONE copy of the relationship logits.

Under ``torch.distributed`` each rank predicts the dataset it is handed; there are no collectives.
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.special import expit

from . import ops
from .config import opt
from .loader import make_loader


class Predictions:
    """numpy arrays in dataset order, named as the outputs of ``lirec_predict_clips``: ``trk``, ``cls``, ``rel`` int32 [n]
    (``rel``: NR = "None", -1 for a recipe without relationship logits), ``score`` float64 [n], ``trk_score`` float64 [n, T],
    ``top_cls`` / ``top_cls_p`` [n, K] (-1 / 0 beyond the classes), ``top_rel`` / ``top_rel_p`` [n, K] or None, ``flags`` int32 [n]
    (bit 0: a NaN among the clip's logits, bit 1: no valid track); ``n_clips``; ``pairs``: ``{hash: (classes in descending order
    of the summed score, summed scores)}`` or None."""
    fields = ops.PREDICT_FIELDS

    def __init__(self, arrays, n_clips, pairs=None):
        for k in self.fields:
            setattr(self, k, arrays.get(k))
        self.n_clips, self.pairs = n_clips, pairs


def pair_scores(rel_logits, hashes):
    """``{hash: (classes, scores)}``: per character pair the float32 sigmoids of its clips' relationship logits, added in clip
    order -- the sums ``RelationshipsAcc.update`` forms -- and the classes in descending order of the sum (stable)."""
    p = expit(np.asarray(rel_logits))                     # (float32 logits from the device: float32 sigmoids and sums)
    sums = {}
    for i, h in enumerate(np.asarray(hashes).reshape(-1)):
        h = int(h)
        if h == -1:
            continue
        sums[h] = sums[h] + p[i] if h in sums else p[i]
    return {h: (np.argsort(-s, kind='stable'), s) for h, s in sums.items()}


def predict(dataset, model, top_k=5, batch_size=None):
    batch_size = opt.batch_size if batch_size is None else batch_size
    loader = make_loader(dataset, batch_size)
    if opt.ints != 1:
        raise ValueError('predict() needs the interaction head (opt.ints == 1)')
    was_training = model.training
    model.eval()
    to_dev = getattr(dataset, 'to_device', None) if (opt.tr_maximize and str(opt.device).startswith('cuda')) else None
    want_pairs = bool(opt.rels_multitask and opt.ctx == 1 and not opt.tr_maximize)
    bufs = dev_rels = None
    at, hashes, have_hash = 0, [], False
    try:
        with torch.no_grad():
            for batch in loader:
                if to_dev is not None:
                    batch = to_dev(batch)
                out = model(batch)
                ints = out['inters']
                C = ints.shape[-1]
                rels = out.get('rels') if opt.ctx == 1 else None
                if opt.tr_maximize:
                    bs = ints.shape[0]
                    T = ints.numel() // (bs * C)
                    mem = batch['mem_mask'].to(ints.device, non_blocking=True).double().contiguous()
                    ints2 = ints.reshape(bs * T, C)
                    rels2 = rels.reshape(bs * T, -1) if rels is not None else None
                else:
                    bs = batch['features'].shape[0]
                    T, mem = 1, None
                    # modalties: one row per clip; int_rels: row 0 of each clip's group of rows, read in place
                    ints2 = ints.reshape(bs, -1, C)[:, 0]
                    rels2 = rels.reshape(bs, -1) if rels is not None else None
                if bufs is None:                          # one set of arrays for the whole dataset
                    n = max(len(dataset), bs)
                    bufs = ops.predict_buffers(n, T, top_k, ints.device, with_rels=rels2 is not None)
                    if want_pairs:
                        dev_rels = torch.empty(n, rels2.shape[1], dtype=rels2.dtype, device=rels2.device)
                if at + bs > bufs['trk'].shape[0]:        # (a dataset that yields more clips than its length)
                    bufs = {k: torch.cat([v, torch.empty_like(v)]) for k, v in bufs.items()}
                    if dev_rels is not None:
                        dev_rels = torch.cat([dev_rels, torch.empty_like(dev_rels)])
                ops.predict_clips(ints2, rels2, mem, B=bs, T=T, K=top_k, loader_types=True,
                                  out={k: v[at:at + bs] for k, v in bufs.items()})
                if want_pairs:                            # the logits wait on the device; the hashes are the loader's host tensors
                    dev_rels[at:at + bs].copy_(rels2)
                    have_hash = have_hash or 'hash_rel' in batch
                    hashes.append(batch['hash_rel'] if 'hash_rel' in batch else torch.full((bs,), -1, dtype=torch.int64))
                at += bs
    finally:
        model.train(was_training)
    if bufs is None:
        predict.last = {}
        return Predictions({}, 0)
    last = {k: v[:at] for k, v in bufs.items()}
    arrays = {k: v.cpu().numpy() for k, v in last.items()}            # one device-to-host copy per field
    pairs = None
    if have_hash:
        pairs = pair_scores(dev_rels[:at].cpu().numpy(), torch.cat([h.reshape(-1).cpu() for h in hashes]).numpy())
    predict.last = dict(last, n_clips=at)
    return Predictions(arrays, at, pairs)


predict.last = {}
